// The prefix-reuse rule of GemmaModel::serveRequests, alone (compiled with the host compiler and -fsanitize=address,undefined and RUN by tests/test_prefix_cache_cpu.py;
// host code only: this file includes nothing but Mila/PrefixCache.h).  The device is a SHADOW CACHE per row: cell p = a hash of tokens[ 0 .. p ], which is what "the KV
// of position p depends on the tokens up to p" means.  Sim runs an admission the way serveRequests does -- plan, beginWrite, fork, the prefill's chunks, extend -- and
// after every operation every claimed position of every row must hold the hash of its claim's prefix.
#include <cstdint>
#include <cstdio>
#include <random>
#include <span>
#include <stdexcept>
#include <vector>

#include "Mila/PrefixCache.h"

using namespace Mila::Dnn;
using Plan = PrefixCache::Plan;
using Tokens = std::vector<int32_t>;

static int failures = 0;
#define CHECK( cond ) do { if ( !( cond ) ) { std::printf( "FAILED line %d: %s\n", __LINE__, #cond ); ++failures; } } while ( 0 )

static uint64_t mix( uint64_t h, int32_t t ) { h ^= static_cast<uint64_t>( static_cast<uint32_t>( t ) ) + 0x9e3779b97f4a7c15ull + ( h << 6 ) + ( h >> 2 ); return h * 0xff51afd7ed558ccdull; }
static constexpr uint64_t kSeed = 0x1234, kGarbage = ~0ull;
/// hashes of every prefix: out[ p ] = hash( tokens[ 0 .. p ] )
static std::vector<uint64_t> prefixHashes( std::span<const int32_t> tokens )
{
    std::vector<uint64_t> out;
    uint64_t h = kSeed;
    for ( int32_t t : tokens ) { h = mix( h, t ); out.push_back( h ); }
    return out;
}

struct Sim
{
    static constexpr int kCapacity = 64, kChunk = 4;
    enum Abort { None, AfterCut, AfterFork, MidPrefill };
    int R;
    PrefixCache cache;
    std::vector<std::vector<uint64_t>> cell;      // the shadow caches
    int64_t forks = 0, in_place = 0, prefilled = 0;

    explicit Sim( int rows ) : R( rows ), cache( rows ), cell( static_cast<size_t>( rows ), std::vector<uint64_t>( kCapacity, kGarbage ) ) {}

    void verify() const
    {
        for ( int r = 0; r < R; ++r )
        {
            const auto want = prefixHashes( cache.claim( r ) );
            CHECK( want.size() <= static_cast<size_t>( kCapacity ) );
            for ( size_t p = 0; p < want.size(); ++p )
                if ( cell[ static_cast<size_t>( r ) ][ p ] != want[ p ] ) { std::printf( "row %d position %zu: the claim says more than the cache holds\n", r, p ); ++failures; return; }
        }
    }
    /// the rule restated without the class: the longest common prefix over all claims, capped, own row first, then the lowest
    Plan expected( int row, const Tokens& prompt, int64_t min_prefix ) const
    {
        int64_t m[ 4 ] = {}, best = 0;
        for ( int s = 0; s < R; ++s )
        {
            const auto& h = cache.claim( s );
            while ( m[ s ] < static_cast<int64_t>( std::min( h.size(), prompt.size() ) ) && h[ static_cast<size_t>( m[ s ] ) ] == prompt[ static_cast<size_t>( m[ s ] ) ] ) ++m[ s ];
            best = std::max( best, m[ s ] );
        }
        const int64_t L = std::min<int64_t>( best, static_cast<int64_t>( prompt.size() ) - 1 );
        if ( L < min_prefix ) return {};
        if ( m[ row ] >= L ) return { row, L };
        for ( int s = 0; s < R; ++s ) if ( m[ s ] >= L ) return { s, L };
        return {};
    }
    /// one admission as serveRequests runs it; abort: where it throws (the shadow cache keeps whatever was written up to there, and some more)
    Plan admit( int row, const Tokens& prompt, int64_t min_prefix = 1, Abort abort = None )
    {
        const Plan pl = cache.plan( row, prompt, min_prefix );
        CHECK( pl == expected( row, prompt, min_prefix ) );
        CHECK( pl.reuse <= static_cast<int64_t>( prompt.size() ) - 1 );
        const auto want = prefixHashes( prompt );
        const size_t L = static_cast<size_t>( pl.reuse );
        auto& mine = cell[ static_cast<size_t>( row ) ];
        if ( L > 0 )      // the donor really holds what the plan takes from it, NOW
            for ( size_t p = 0; p < L; ++p ) CHECK( cell[ static_cast<size_t>( pl.donor ) ][ p ] == want[ p ] );
        cache.beginWrite( row, pl.donor == row ? L : 0 );
        verify();
        if ( abort == AfterCut ) return pl;
        if ( L > 0 && pl.donor != row )
        {
            for ( size_t p = 0; p < L; ++p ) mine[ p ] = cell[ static_cast<size_t>( pl.donor ) ][ p ];
            cache.extend( row, std::span<const int32_t>( prompt ).first( L ) );
            ++forks;
        }
        else if ( L > 0 ) ++in_place;
        verify();
        if ( abort == AfterFork ) return pl;
        for ( size_t p0 = L; p0 < prompt.size(); p0 += kChunk )
        {
            const size_t c = std::min<size_t>( kChunk, prompt.size() - p0 );
            if ( abort == MidPrefill && p0 > L )      // a chunk that died half way: positions written, never claimed
            {
                mine[ p0 ] = kGarbage - 1;
                verify();
                return pl;
            }
            for ( size_t p = p0; p < p0 + c; ++p ) mine[ p ] = want[ p ];
            cache.extend( row, std::span<const int32_t>( prompt ).subspan( p0, c ) );
            prefilled += static_cast<int64_t>( c );
            verify();
        }
        CHECK( cache.claim( row ) == prompt );
        return pl;
    }
    /// the identical-prompt rule of RequestQueue: a whole fork, logits and all, no prefill
    void forkWhole( int src, int dst, const Tokens& prompt )
    {
        CHECK( cache.claim( src ) == prompt );
        cache.beginWrite( dst, 0 );
        for ( size_t p = 0; p < prompt.size(); ++p ) cell[ static_cast<size_t>( dst ) ][ p ] = cell[ static_cast<size_t>( src ) ][ p ];
        cache.extend( dst, prompt );
        verify();
    }
    /// a rows step feeds `token` into live row r: its KV lands at the row's position
    void step( int row, int32_t token )
    {
        const auto& h = cache.claim( row );
        const size_t p = h.size();
        cell[ static_cast<size_t>( row ) ][ p ] = mix( p ? prefixHashes( h ).back() : kSeed, token );
        cache.fed( row, token );
        verify();
    }
};

static void the_last_position_is_always_prefilled()
{
    Sim s( 2 );
    const Tokens p{ 5, 6, 7, 8 };
    CHECK( ( s.admit( 0, p ) == Plan{ -1, 0 } ) );
    CHECK( ( s.cache.plan( 1, p ) == Plan{ 0, 3 } ) );                          // the same prompt again: len - 1
    CHECK( ( s.cache.plan( 0, p ) == Plan{ 0, 3 } ) );                          // ... in place
    CHECK( ( s.cache.plan( 1, Tokens{ 5, 6 } ) == Plan{ 0, 1 } ) );              // a shorter one: still its last position
    CHECK( ( s.cache.plan( 1, Tokens{ 5 } ) == Plan{ -1, 0 } ) );                // one token: nothing to reuse
    CHECK( ( s.cache.plan( 1, Tokens{ 5, 6, 7, 8, 9 } ) == Plan{ 0, 4 } ) );     // a longer one: the donor's whole prompt
    s.step( 0, 9 );
    s.step( 0, 4 );
    CHECK( ( s.cache.plan( 1, Tokens{ 5, 6, 7, 8, 9, 4, 1 } ) == Plan{ 0, 6 } ) );      // into the donor's decoded tokens
    CHECK( ( s.cache.plan( 1, Tokens{ 5, 6, 7, 8, 9, 3 } ) == Plan{ 0, 5 } ) );
}

static void ties_go_to_the_own_row_then_to_the_lowest()
{
    Sim s( 4 );
    s.admit( 2, Tokens{ 1, 2, 3, 9 } );
    s.forkWhole( 2, 1, Tokens{ 1, 2, 3, 9 } );
    s.forkWhole( 2, 3, Tokens{ 1, 2, 3, 9 } );
    const Tokens q{ 1, 2, 3, 4 };
    CHECK( ( s.cache.plan( 0, q ) == Plan{ 1, 3 } ) );      // rows 1, 2, 3 tie: the lowest
    CHECK( ( s.cache.plan( 3, q ) == Plan{ 3, 3 } ) );      // the own row ties: in place
    CHECK( ( s.cache.plan( 2, q ) == Plan{ 2, 3 } ) );
    // a longer match elsewhere beats the own row's shorter one ...
    s.admit( 0, Tokens{ 1, 2, 7, 7 } );
    CHECK( ( s.cache.plan( 0, q ) == Plan{ 1, 3 } ) );
    // ... but the cap can make the own row's match enough: both reach len - 1 = 2
    CHECK( ( s.cache.plan( 0, Tokens{ 1, 2, 3 } ) == Plan{ 0, 2 } ) );
    const int64_t forks = s.forks;
    s.admit( 3, q );
    CHECK( s.forks == forks && s.in_place == 1 );
}

static void min_prefix_refuses_short_matches()
{
    Sim s( 2 );
    s.admit( 0, Tokens{ 1, 2, 3, 4, 5 } );
    const Tokens q{ 1, 2, 3, 8, 8 };
    CHECK( ( s.cache.plan( 1, q, 3 ) == Plan{ 0, 3 } ) );
    CHECK( ( s.cache.plan( 1, q, 4 ) == Plan{ -1, 0 } ) );
    CHECK( ( s.cache.plan( 0, q, 4 ) == Plan{ -1, 0 } ) );      // in place too
    const int64_t before = s.prefilled;
    CHECK( ( s.admit( 1, q, 4 ) == Plan{ -1, 0 } ) );
    CHECK( s.prefilled == before + 5 );
    bool threw = false;
    try { (void)s.cache.plan( 1, q, 0 ); } catch ( const std::invalid_argument& ) { threw = true; }
    CHECK( threw );
    threw = false;
    try { (void)s.cache.plan( 1, Tokens{}, 1 ); } catch ( const std::invalid_argument& ) { threw = true; }
    CHECK( threw );
    threw = false;
    try { (void)s.cache.plan( 2, q, 1 ); } catch ( const std::invalid_argument& ) { threw = true; }
    CHECK( threw );
    threw = false;
    try { s.cache.beginWrite( 0, 99 ); } catch ( const std::logic_error& ) { threw = true; }
    CHECK( threw );
}

static void a_swap_in_one_wave_never_reads_a_cut_claim()
{
    // rows 0 and 1 are free and hold A.. and B..; the wave admits a B-request into row 0 and an A-request into row 1: each one's best donor is the other's row.
    const Tokens A{ 1, 1, 1, 1, 2 }, B{ 3, 3, 3, 3, 4 }, qB{ 3, 3, 3, 3, 5, 6 }, qA{ 1, 1, 1, 1, 7, 8 };
    Sim s( 2 );
    s.admit( 0, A );
    s.admit( 1, B );
    // planned up front, the second plan would name row 0 -- which the first admission overwrites
    CHECK( ( s.cache.plan( 0, qB ) == Plan{ 1, 4 } ) );
    CHECK( ( s.cache.plan( 1, qA ) == Plan{ 0, 4 } ) );
    // sequentially: the first forks from row 1; then row 0 no longer claims A, and the second finds nothing
    CHECK( ( s.admit( 0, qB ) == Plan{ 1, 4 } ) );
    CHECK( ( s.admit( 1, qA ) == Plan{ -1, 0 } ) );      // (admit() also checked that a planned donor holds the bits at that moment)
    CHECK( s.cache.claim( 0 ) == qB && s.cache.claim( 1 ) == qA );
    // and a later admission of the round sees an earlier one's fresh whole prompt
    Sim t( 3 );
    t.admit( 0, Tokens{ 9, 9, 9, 1 } );
    CHECK( ( t.admit( 1, Tokens{ 9, 9, 9, 2, 2 } ) == Plan{ 0, 3 } ) );
    CHECK( ( t.admit( 2, Tokens{ 9, 9, 9, 2, 3 } ) == Plan{ 1, 4 } ) );
}

static void the_identical_prompt_rule_leaves_the_same_claims()
{
    const Tokens p{ 4, 5, 6, 7, 8, 9 };
    Sim forked( 3 ), planned( 3 );
    forked.admit( 0, p );
    forked.forkWhole( 0, 1, p );
    forked.forkWhole( 0, 2, p );
    planned.admit( 0, p );
    CHECK( ( planned.admit( 1, p ) == Plan{ 0, 5 } ) );
    CHECK( ( planned.admit( 2, p ) == Plan{ 0, 5 } ) );
    for ( int r = 0; r < 3; ++r ) CHECK( forked.cache.claim( r ) == planned.cache.claim( r ) && forked.cache.claim( r ) == p );
    CHECK( forked.cell == planned.cell );
}

static void aborted_admissions_leave_nothing_stale()
{
    const Tokens A{ 1, 2, 3, 4, 5, 6, 7, 8, 9 };
    for ( auto where : { Sim::AfterCut, Sim::AfterFork, Sim::MidPrefill } )
    {
        Sim s( 2 );
        s.admit( 0, A );
        s.admit( 1, Tokens{ 7, 7, 7 } );
        const Tokens q{ 1, 2, 3, 4, 5, 5, 5, 5, 5, 5, 5 };
        s.admit( 1, q, 1, where );
        const size_t held = s.cache.claim( 1 ).size();
        CHECK( where == Sim::AfterCut ? held == 0 : where == Sim::AfterFork ? held == 5 : held == 9 );
        s.cache.invalidate( 1 );
        CHECK( s.cache.claim( 1 ).empty() && s.cache.claim( 0 ) == A );
        s.cache.clear();
        CHECK( s.cache.claim( 0 ).empty() );
        s.verify();
    }
}

static void a_random_schedule( uint64_t seed, int R )
{
    std::mt19937_64 rng( seed );
    auto below = [&]( int n ) { return static_cast<int>( rng() % static_cast<uint64_t>( n ) ); };
    Sim s( R );
    std::vector<char> live( static_cast<size_t>( R ), 0 );
    std::vector<int32_t> pending( static_cast<size_t>( R ), 0 );      // the token a live row sampled last: the next step feeds it
    for ( int op = 0; op < 600; ++op )
    {
        const int kind = below( 10 );
        if ( kind < 4 )      // a round: every free row, lowest first, takes a request -- now and then one that dies on the way
        {
            for ( int r = 0; r < R; ++r )
            {
                if ( live[ static_cast<size_t>( r ) ] || below( 3 ) == 0 ) continue;
                Tokens prompt;
                if ( below( 4 ) )      // starts like something a row holds: a claim's prefix, then a tail
                {
                    const auto& h = s.cache.claim( below( R ) );
                    if ( !h.empty() ) prompt.assign( h.begin(), h.begin() + 1 + below( static_cast<int>( h.size() ) ) );
                }
                if ( prompt.size() > 20 ) prompt.resize( 20 );
                for ( int k = below( 6 ) + ( prompt.empty() ? 1 : 0 ); k > 0; --k ) prompt.push_back( below( 3 ) );
                const auto abort = below( 8 ) == 0 ? static_cast<Sim::Abort>( 1 + below( 3 ) ) : Sim::None;
                s.admit( r, prompt, 1 + below( 3 ), abort );
                if ( abort != Sim::None ) { if ( below( 2 ) ) s.cache.clear(); continue; }      // (serveRequests clears everything; the rule alone must hold without)
                live[ static_cast<size_t>( r ) ] = 1;
                pending[ static_cast<size_t>( r ) ] = below( 3 );
            }
        }
        else if ( kind < 9 )      // a step over the live rows, then some retire
        {
            for ( int r = 0; r < R; ++r )
            {
                if ( !live[ static_cast<size_t>( r ) ] ) continue;
                if ( s.cache.claim( r ).size() + 1 >= static_cast<size_t>( Sim::kCapacity ) ) { live[ static_cast<size_t>( r ) ] = 0; continue; }
                s.step( r, pending[ static_cast<size_t>( r ) ] );
                pending[ static_cast<size_t>( r ) ] = below( 3 );
                if ( below( 4 ) == 0 ) live[ static_cast<size_t>( r ) ] = 0;      // its last sample is never fed
            }
        }
        else      // a free row is forgotten (a live row's claim is what fed() appends to: it is never dropped alone)
        {
            const int r = below( R );
            if ( !live[ static_cast<size_t>( r ) ] ) s.cache.invalidate( r );
        }
        s.verify();
    }
    CHECK( s.forks > 0 && s.in_place > 0 && s.prefilled > 0 );
}

int main()
{
    the_last_position_is_always_prefilled();
    ties_go_to_the_own_row_then_to_the_lowest();
    min_prefix_refuses_short_matches();
    a_swap_in_one_wave_never_reads_a_cut_claim();
    the_identical_prompt_rule_leaves_the_same_claims();
    aborted_admissions_leave_nothing_stale();
    for ( int R = 2; R <= 4; ++R )
        for ( uint64_t seed = 1; seed <= 4; ++seed ) a_random_schedule( seed * 7919 + static_cast<uint64_t>( R ), R );
    bool threw = false;
    try { PrefixCache bad( 5 ); } catch ( const std::invalid_argument& ) { threw = true; }
    CHECK( threw );
    if ( failures ) { std::printf( "%d failures\n", failures ); return 1; }
    std::printf( "prefix cache OK\n" );
    return 0;
}
