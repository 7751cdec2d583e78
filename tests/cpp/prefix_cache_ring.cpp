// The prefix-reuse rule with a VALID-FROM bound (Mila/PrefixCache.h, RINGS), alone: compiled with the host compiler and -fsanitize=address,undefined and RUN by
// tests/test_prefix_cache_ring_cpu.py; host code only, nothing but Mila/PrefixCache.h.  The device is a SHADOW per row with two caches: a flat one (the global layers:
// cell p = a hash of tokens[ 0 .. p ]) and a ring of `capacity` cells (the sliding-window layers: cell p % capacity = (p, that hash)).  Sim runs what serveRequests runs
// on a ring model -- plan, beginWrite, the band fork + adopt, the suffix prefill in chunks of capacity - window + 1, steps (which also write the stale token of every row
// that is in the step but not live, at its position word), retirements, aborted admissions, rewinds -- and after every write, for every length L a continuation may start
// from (every L the rule calls usable, and a live row's own length), the ring cells of [max( 0, L - window + 1 ), L) must hold the right (position, hash).  One run with the
// bound switched off must make the same shadow report a stale cell: otherwise it proves nothing.
#include <algorithm>
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
static std::vector<uint64_t> prefixHashes( std::span<const int32_t> tokens )
{
    std::vector<uint64_t> out;
    uint64_t h = kSeed;
    for ( int32_t t : tokens ) { h = mix( h, t ); out.push_back( h ); }
    return out;
}

struct Cell { int64_t pos = -1; uint64_t hash = kGarbage; bool operator==( const Cell& ) const = default; };

struct Sim
{
    static constexpr int64_t kMaxLen = 72;      // the flat caches' capacity (the context)
    enum Abort { None, AfterCut, AfterFork, MidPrefill };
    int R;
    int64_t W, CAP, chunk;      // W == 0: no rings (the 0 / 0 geometry)
    bool bound;                 // false: the cache is asked as if there were no rings (the self-check)
    PrefixCache cache;
    std::vector<std::vector<uint64_t>> flat;
    std::vector<std::vector<Cell>> ring;
    std::vector<int64_t> hi, fr, word;      // the test's own account of high / from, and each row's position word
    std::vector<char> live;
    int64_t stale = 0, forks = 0, in_place = 0, prefilled = 0, refused = 0, rewinds = 0;

    Sim( int rows, int64_t window, int64_t capacity, bool with_bound = true )
        : R( rows ), W( window ), CAP( capacity ), chunk( window > 0 ? capacity - window + 1 : 4 ), bound( with_bound ),
          cache( rows, with_bound ? window : 0, with_bound ? capacity : 0 ), flat( static_cast<size_t>( rows ), std::vector<uint64_t>( kMaxLen + 1, kGarbage ) ),
          ring( static_cast<size_t>( rows ), std::vector<Cell>( static_cast<size_t>( std::max<int64_t>( capacity, 1 ) ) ) ), hi( static_cast<size_t>( rows ), 0 ), fr( static_cast<size_t>( rows ), 0 ),
          word( static_cast<size_t>( rows ), 0 ), live( static_cast<size_t>( rows ), 0 ) {}

    void put( int r, int64_t p, uint64_t h )
    {
        flat[ static_cast<size_t>( r ) ][ static_cast<size_t>( p ) ] = h;
        if ( W > 0 ) ring[ static_cast<size_t>( r ) ][ static_cast<size_t>( p % CAP ) ] = Cell{ p, h };
        hi[ static_cast<size_t>( r ) ] = std::max( hi[ static_cast<size_t>( r ) ], p + 1 );
    }
    /// the rule restated without the class
    bool usableHere( int s, int64_t L ) const
    {
        if ( W <= 0 || !bound ) return true;
        const int64_t high = hi[ static_cast<size_t>( s ) ], from = std::max<int64_t>( { 0, fr[ static_cast<size_t>( s ) ], high - CAP + 1 } );
        return std::max<int64_t>( 0, L - W + 1 ) >= from;
    }
    /// the ring cells a continuation of row r from L reads before it writes them itself
    bool bandIntact( int r, int64_t L, const std::vector<uint64_t>& want ) const
    {
        if ( W <= 0 ) return true;
        for ( int64_t p = std::max<int64_t>( 0, L - W + 1 ); p < L; ++p )
            if ( !( ring[ static_cast<size_t>( r ) ][ static_cast<size_t>( p % CAP ) ] == Cell{ p, want[ static_cast<size_t>( p ) ] } ) ) return false;
        return true;
    }
    void verify()
    {
        for ( int r = 0; r < R; ++r )
        {
            const auto& h = cache.claim( r );
            const auto want = prefixHashes( h );
            const int64_t n = static_cast<int64_t>( want.size() );
            CHECK( n <= kMaxLen );
            if ( bound ) CHECK( cache.high( r ) == ( W > 0 ? hi[ static_cast<size_t>( r ) ] : cache.high( r ) ) );
            for ( int64_t p = 0; p < n; ++p )
                if ( flat[ static_cast<size_t>( r ) ][ static_cast<size_t>( p ) ] != want[ static_cast<size_t>( p ) ] ) { std::printf( "row %d position %lld: the claim says more than the flat cache holds\n", r, static_cast<long long>( p ) ); ++failures; return; }
            for ( int64_t L = 1; L <= n; ++L )
            {
                const bool asked = cache.usable( r, L );
                CHECK( asked == usableHere( r, L ) );
                if ( ( asked || ( live[ static_cast<size_t>( r ) ] && L == n ) ) && !bandIntact( r, L, want ) ) ++stale;
            }
        }
    }
    Plan expected( int row, const Tokens& prompt, int64_t min_prefix ) const
    {
        int64_t m[ 4 ] = {}, best = 0;
        const int64_t last = static_cast<int64_t>( prompt.size() ) - 1;
        for ( int s = 0; s < R; ++s )
        {
            const auto& h = cache.claim( s );
            while ( m[ s ] < static_cast<int64_t>( std::min( h.size(), prompt.size() ) ) && h[ static_cast<size_t>( m[ s ] ) ] == prompt[ static_cast<size_t>( m[ s ] ) ] ) ++m[ s ];
            if ( !usableHere( s, std::min( m[ s ], last ) ) ) m[ s ] = 0;
            best = std::max( best, m[ s ] );
        }
        const int64_t L = std::min( best, last );
        if ( L < min_prefix ) return {};
        if ( m[ row ] >= L ) return { row, L };
        for ( int s = 0; s < R; ++s ) if ( m[ s ] >= L ) return { s, L };
        return {};
    }
    /// kv_rows_fork_layers_band_bf16 in the shadow: the flat prefix, and the ring CELLS of the band as they are
    void bandFork( int src, int dst, int64_t L )
    {
        for ( int64_t p = 0; p < L; ++p ) flat[ static_cast<size_t>( dst ) ][ static_cast<size_t>( p ) ] = flat[ static_cast<size_t>( src ) ][ static_cast<size_t>( p ) ];
        if ( W > 0 )
            for ( int64_t p = std::max<int64_t>( 0, L - W ); p < L; ++p ) ring[ static_cast<size_t>( dst ) ][ static_cast<size_t>( p % CAP ) ] = ring[ static_cast<size_t>( src ) ][ static_cast<size_t>( p % CAP ) ];
        hi[ static_cast<size_t>( dst ) ] = L;
        fr[ static_cast<size_t>( dst ) ] = W > 0 ? std::max<int64_t>( 0, L - W + 1 ) : 0;
    }
    Plan admit( int row, const Tokens& prompt, int64_t min_prefix = 1, Abort abort = None )
    {
        const Plan pl = cache.plan( row, prompt, min_prefix );
        CHECK( pl == expected( row, prompt, min_prefix ) );
        const auto want = prefixHashes( prompt );
        const int64_t L = pl.reuse, n = static_cast<int64_t>( prompt.size() );
        if ( L > 0 && !bandIntact( pl.donor, L, want ) ) ++stale;      // the donor holds what the plan takes from it, NOW
        cache.beginWrite( row, pl.donor == row ? static_cast<size_t>( L ) : 0 );
        if ( pl.donor != row || L == 0 ) hi[ static_cast<size_t>( row ) ] = fr[ static_cast<size_t>( row ) ] = 0;
        live[ static_cast<size_t>( row ) ] = 0;
        verify();
        if ( abort == AfterCut ) return pl;
        if ( L > 0 && pl.donor != row )
        {
            bandFork( pl.donor, row, L );
            cache.adopt( row, std::span<const int32_t>( prompt ).first( static_cast<size_t>( L ) ) );
            ++forks;
        }
        else if ( L > 0 ) ++in_place;
        verify();
        if ( abort == AfterFork ) return pl;
        for ( int64_t p0 = L; p0 < n; p0 += chunk )
        {
            const int64_t c = std::min( chunk, n - p0 );
            if ( abort == MidPrefill && p0 > L )      // a chunk that died half way: written, never claimed (serveRequests then forgets every claim: the schedule does)
            {
                flat[ static_cast<size_t>( row ) ][ static_cast<size_t>( p0 ) ] = kGarbage - 1;
                if ( W > 0 ) ring[ static_cast<size_t>( row ) ][ static_cast<size_t>( p0 % CAP ) ] = Cell{ -3, kGarbage - 1 };
                return pl;
            }
            for ( int64_t p = p0; p < p0 + c; ++p ) put( row, p, want[ static_cast<size_t>( p ) ] );
            // the chunk's attention runs after its writes: row p0 reads down to p0 - W + 1, and the chunk's own cells must not have taken those
            if ( !bandIntact( row, p0 + c, want ) || !bandIntact( row, p0, want ) ) ++stale;
            cache.extend( row, std::span<const int32_t>( prompt ).subspan( static_cast<size_t>( p0 ), static_cast<size_t>( c ) ) );
            prefilled += c;
            verify();
        }
        CHECK( cache.claim( row ) == prompt );
        word[ static_cast<size_t>( row ) ] = n;
        live[ static_cast<size_t>( row ) ] = 1;
        return pl;
    }
    /// the identical-prompt rule: forkRow, logits and all
    void forkWhole( int src, int dst, const Tokens& prompt )
    {
        CHECK( cache.claim( src ) == prompt );
        cache.beginWrite( dst, 0 );
        bandFork( src, dst, static_cast<int64_t>( prompt.size() ) );
        cache.adopt( dst, prompt );
        word[ static_cast<size_t>( dst ) ] = static_cast<int64_t>( prompt.size() );
        live[ static_cast<size_t>( dst ) ] = 1;
        verify();
    }
    /// one rows step over every row: a live row is fed its token at its position; a row that is not live has its stale token's K / V written at its position word
    void step( const std::vector<int32_t>& token )
    {
        for ( int r = 0; r < R; ++r )
        {
            const int64_t p = word[ static_cast<size_t>( r ) ];
            if ( !live[ static_cast<size_t>( r ) ] )
            {
                if ( p < kMaxLen ) flat[ static_cast<size_t>( r ) ][ static_cast<size_t>( p ) ] = kGarbage - 2;
                if ( W > 0 ) ring[ static_cast<size_t>( r ) ][ static_cast<size_t>( p % CAP ) ] = Cell{ -2, kGarbage - 2 };
                continue;
            }
            const auto& h = cache.claim( r );
            CHECK( static_cast<int64_t>( h.size() ) == p );
            put( r, p, mix( p ? prefixHashes( h ).back() : kSeed, token[ static_cast<size_t>( r ) ] ) );
            cache.fed( r, token[ static_cast<size_t>( r ) ] );
            word[ static_cast<size_t>( r ) ] = p + 1;
        }
        verify();
    }
    void retire( int r ) { live[ static_cast<size_t>( r ) ] = 0; }
    /// rewindKvCacheRow: the row goes on from L, if the rule lets it
    bool rewind( int r, int64_t L )
    {
        if ( !cache.usable( r, L ) ) { ++refused; return false; }
        cache.beginWrite( r, static_cast<size_t>( L ) );
        word[ static_cast<size_t>( r ) ] = L;
        ++rewinds;
        verify();
        return true;
    }
};

static Tokens iota( int n, int32_t first = 1 ) { Tokens t; for ( int i = 0; i < n; ++i ) t.push_back( first + i ); return t; }
static Tokens cat( Tokens a, const Tokens& b ) { a.insert( a.end(), b.begin(), b.end() ); return a; }

static void a_donor_just_inside_and_just_outside_the_slack( int64_t CAP )
{
    const int64_t W = 8, slack = CAP - W;
    for ( int64_t extra : { int64_t( 0 ), int64_t( 1 ) } )
    {
        Sim s( 2, W, CAP );
        const int64_t L = 20;
        s.admit( 0, iota( static_cast<int>( L ) ) );
        for ( int64_t k = 0; k < slack + extra; ++k ) s.step( { 7, 0 } );      // high - L == slack (+ 1)
        CHECK( s.cache.high( 0 ) - L == slack + extra );
        const Tokens q = cat( iota( static_cast<int>( L ) ), Tokens{ 90, 91 } );
        const Plan pl = s.cache.plan( 1, q );
        if ( extra == 0 ) CHECK( ( pl == Plan{ 0, L } ) ); else CHECK( ( pl == Plan{ -1, 0 } ) );
        s.retire( 0 );
        s.step( { 0, 0 } );      // the retired donor's stale token lands in its ring: the answer stands
        CHECK( ( s.admit( 1, q ) == pl ) );
        CHECK( s.stale == 0 );
    }
}

static void a_forked_row_donates_no_shorter_prefix_unless_it_fits_the_window()
{
    Sim s( 3, 8, 11 );
    const Tokens p = iota( 20 );
    s.admit( 0, p );
    s.forkWhole( 0, 1, p );      // row 1 holds [12, 20) on the rings
    CHECK( s.cache.validFrom( 1 ) == 13 && s.cache.validFrom( 0 ) == 10 );
    s.retire( 0 );
    s.cache.invalidate( 0 );      // only the forked row is left to ask
    CHECK( ( s.cache.plan( 2, cat( iota( 15 ), Tokens{ 77, 78 } ) ) == Plan{ -1, 0 } ) );      // 15 - 8 < 20 - 8
    CHECK( ( s.cache.plan( 2, cat( p, Tokens{ 77 } ) ) == Plan{ 1, 20 } ) );                    // its whole length
    CHECK( ( s.cache.plan( 2, p ) == Plan{ -1, 0 } ) );                                          // len - 1 = 19: 19 - 8 < 20 - 8
    Sim t( 3, 8, 11 );
    const Tokens shortp = iota( 7 );
    t.admit( 0, shortp );
    t.forkWhole( 0, 1, shortp );      // len <= window: valid from 0, any prefix may be donated
    CHECK( t.cache.validFrom( 1 ) == 0 );
    t.cache.invalidate( 0 );
    CHECK( ( t.admit( 2, cat( iota( 4 ), Tokens{ 50, 51 } ) ) == Plan{ 1, 4 } ) );
    CHECK( s.stale == 0 && t.stale == 0 );
}

static void in_place_reuse_counts_the_stale_tail()
{
    Sim s( 2, 8, 11 );
    s.admit( 0, iota( 24 ) );
    s.retire( 0 );
    // a shorter rewrite in place: 22 of the 24 stay (24 - 22 <= 3), and the tail [22, 24) is still in the ring
    CHECK( ( s.admit( 0, cat( iota( 22 ), Tokens{ 60 } ) ) == Plan{ 0, 22 } ) );
    CHECK( s.cache.high( 0 ) == 24 && s.cache.claim( 0 ).size() == 23 );
    s.retire( 0 );
    // 20 would pass against the claim's 23 (23 - 20 = 3), not against high = 24 (24 - 20 > 11 - 8)
    CHECK( !s.cache.usable( 0, 20 ) && s.cache.usable( 0, 21 ) );
    CHECK( ( s.cache.plan( 0, cat( iota( 20 ), Tokens{ 61, 62 } ) ) == Plan{ -1, 0 } ) );
    CHECK( ( s.admit( 0, cat( iota( 21 ), Tokens{ 61, 62 } ) ) == Plan{ 0, 21 } ) );
    // written up to exactly the capacity: nothing has wrapped, but the row's position word sits on cell 0 -- a prefix shorter than the window is refused
    Sim t( 2, 8, 11 );
    t.admit( 0, iota( 11 ) );
    t.retire( 0 );
    CHECK( !t.cache.usable( 0, 5 ) && t.cache.usable( 0, 8 ) );
    t.step( { 0, 0 } );
    CHECK( ( t.admit( 1, cat( iota( 5 ), Tokens{ 70, 71 } ) ) == Plan{ -1, 0 } ) );
    CHECK( s.stale == 0 && t.stale == 0 );
}

struct Counts { int64_t stale, forks, in_place, refused, rewinds; };
static Counts a_random_schedule( uint64_t seed, int R, int64_t W, int64_t CAP, bool bound )
{
    std::mt19937_64 rng( seed );
    auto below = [&]( int n ) { return static_cast<int>( rng() % static_cast<uint64_t>( n ) ); };
    Sim s( R, W, CAP, bound );
    for ( int op = 0; op < 700; ++op )
    {
        const int kind = below( 12 );
        if ( kind < 4 )
        {
            for ( int r = 0; r < R; ++r )
            {
                if ( s.live[ static_cast<size_t>( r ) ] || below( 3 ) == 0 ) continue;
                Tokens prompt;
                if ( below( 5 ) )
                {
                    const auto& h = s.cache.claim( below( R ) );
                    if ( !h.empty() ) prompt.assign( h.begin(), h.begin() + 1 + below( static_cast<int>( h.size() ) ) );
                }
                if ( prompt.size() > 40 ) prompt.resize( 40 );
                for ( int k = below( 14 ) + ( prompt.empty() ? 1 : 0 ); k > 0; --k ) prompt.push_back( below( 3 ) );
                const auto abort = below( 8 ) == 0 ? static_cast<Sim::Abort>( 1 + below( 3 ) ) : Sim::None;
                const int64_t min_prefix = 1 + below( 3 );
                // the identical-prompt rule now and then: a live row that holds exactly this prompt and has not stepped
                int same = -1;
                for ( int q = 0; q < R; ++q ) if ( q != r && s.live[ static_cast<size_t>( q ) ] && s.cache.claim( q ) == prompt && s.hi[ static_cast<size_t>( q ) ] == static_cast<int64_t>( prompt.size() ) ) same = q;
                if ( same >= 0 && abort == Sim::None ) { s.forkWhole( same, r, prompt ); continue; }
                (void)s.admit( r, prompt, min_prefix, abort );      // (admit() holds the plan against the rule restated: with 0 / 0 that is the flat rule)
                if ( abort != Sim::None )      // as serveRequests does after any exception: every claim forgotten, the call over (an aborted row's position word is whatever it was)
                {
                    s.cache.clear();
                    for ( int q = 0; q < R; ++q ) s.retire( q );
                    break;
                }
            }
        }
        else if ( kind < 10 )
        {
            std::vector<int32_t> tok( static_cast<size_t>( R ) );
            for ( auto& t : tok ) t = below( 3 );
            for ( int r = 0; r < R; ++r ) if ( s.live[ static_cast<size_t>( r ) ] && s.word[ static_cast<size_t>( r ) ] + 1 >= Sim::kMaxLen ) s.retire( r );
            s.step( tok );
            for ( int r = 0; r < R; ++r ) if ( s.live[ static_cast<size_t>( r ) ] && below( 4 ) == 0 ) s.retire( r );
        }
        else if ( kind == 10 )
        {
            const int r = below( R );
            if ( !s.live[ static_cast<size_t>( r ) ] ) s.cache.invalidate( r );
        }
        else      // a live row is rewound by a few positions, where the rule allows
        {
            const int r = below( R );
            const int64_t n = static_cast<int64_t>( s.cache.claim( r ).size() );
            if ( s.live[ static_cast<size_t>( r ) ] && n > 2 && W > 0 ) (void)s.rewind( r, std::max<int64_t>( 1, n - 1 - below( 5 ) ) );
        }
        s.verify();
    }
    return { s.stale, s.forks, s.in_place, s.refused, s.rewinds };
}

int main()
{
    for ( int64_t cap : { int64_t( 11 ), int64_t( 16 ), int64_t( 23 ) } ) a_donor_just_inside_and_just_outside_the_slack( cap );
    a_forked_row_donates_no_shorter_prefix_unless_it_fits_the_window();
    in_place_reuse_counts_the_stale_tail();
    int64_t unbounded_stale = 0;
    Counts seen{};
    for ( int64_t cap : { int64_t( 11 ), int64_t( 16 ), int64_t( 23 ) } )
        for ( int R = 2; R <= 4; ++R )
            for ( uint64_t seed = 1; seed <= 4; ++seed )
            {
                const Counts c = a_random_schedule( seed * 7919 + static_cast<uint64_t>( R ) + static_cast<uint64_t>( cap ) * 31, R, 8, cap, true );
                if ( c.stale ) { std::printf( "capacity %lld rows %d seed %llu: %lld stale cells under the bound\n", static_cast<long long>( cap ), R, static_cast<unsigned long long>( seed ), static_cast<long long>( c.stale ) ); ++failures; }
                seen.forks += c.forks; seen.in_place += c.in_place; seen.refused += c.refused; seen.rewinds += c.rewinds;
                if ( seed == 1 ) unbounded_stale += a_random_schedule( seed * 7919 + static_cast<uint64_t>( R ) + static_cast<uint64_t>( cap ) * 31, R, 8, cap, false ).stale;
            }
    CHECK( seen.forks > 0 && seen.in_place > 0 && seen.refused > 0 && seen.rewinds > 0 );
    CHECK( unbounded_stale > 0 );      // the self-check: without the bound the shadow sees stale cells
    for ( int R = 2; R <= 4; ++R ) CHECK( a_random_schedule( 4242 + static_cast<uint64_t>( R ), R, 0, 0, true ).stale == 0 );      // 0 / 0: the flat rule, answer for answer
    for ( auto bad : { std::pair<int64_t, int64_t>{ 8, 0 }, { 0, 11 }, { 8, 7 }, { -1, -1 } } )
    {
        bool threw = false;
        try { PrefixCache c( 2, bad.first, bad.second ); } catch ( const std::invalid_argument& ) { threw = true; }
        CHECK( threw );
    }
    if ( failures ) { std::printf( "%d failures\n", failures ); return 1; }
    std::printf( "prefix cache ring OK (%lld stale cells seen with the bound off)\n", static_cast<long long>( unbounded_stale ) );
    return 0;
}
