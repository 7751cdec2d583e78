// Host-only facts of constrained speculative decode (compiled AND run, without a GPU, by tests/test_token_automaton_forced_cpu.py with the host flags of
// mila_amd/build.py): GenerateParams::speculate_constrained and SpeculationStats::forced / forced_accepted exist; TokenAutomaton::forcedTokens is the brute-force
// answer -- the one token of a state with a transition and a finite bias, else -1 -- on random small automata (vocab <= 40, S <= 6), without a bias, with bans, under an
// allow-list and before a min_tokens restore; and on a hand-made automaton a state is forced only because of a ban.
#include <cmath>
#include <cstdio>
#include <random>
#include <type_traits>
#include <vector>

#include "Mila/GemmaModel.h"

using namespace Mila::Dnn;

static_assert( std::is_same_v<decltype( GenerateParams::speculate_constrained ), bool> );
static_assert( std::is_same_v<decltype( SpeculationStats::forced ), uint64_t> && std::is_same_v<decltype( SpeculationStats::forced_accepted ), uint64_t> );

// the dense table a plan stands for
static std::vector<float> denseBias( const TokenBiasPlan& plan, int64_t vocab )
{
    std::vector<float> t( static_cast<size_t>( vocab ), plan.active ? plan.fill : 0.0f );
    if ( plan.active )
        for ( size_t j = 0; j < plan.ids.size(); ++j ) t[ static_cast<size_t>( plan.ids[ j ] ) ] = plan.values[ j ];
    return t;
}
static std::vector<int32_t> bruteForce( const TokenAutomaton& a, const TokenBiasPlan& plan )
{
    const std::vector<float> bias = denseBias( plan, a.vocab() );
    std::vector<int32_t> forced( static_cast<size_t>( a.num_states ), -1 );
    for ( int s = 0; s < a.num_states; ++s )
    {
        int n = 0;
        int32_t last = -1;
        for ( int32_t t = 0; t < a.vocab(); ++t )
            if ( a.allows( s, t ) && std::isfinite( bias[ static_cast<size_t>( t ) ] ) ) { ++n; last = t; }
        if ( n == 1 ) forced[ static_cast<size_t>( s ) ] = last;
    }
    return forced;
}

int main()
{
    int bad = 0;
    auto expect = [&]( bool ok, const char* what ) { if ( !ok ) { std::printf( "FAILED: %s\n", what ); ++bad; } };
    constexpr uint16_t F = TokenAutomaton::FORBIDDEN;
    expect( !GenerateParams{}.speculate_constrained, "speculate_constrained is off by default" );
    std::mt19937 rng( 20240917 );
    auto below = [&]( int n ) { return static_cast<int>( rng() % static_cast<unsigned>( n ) ); };
    int forced_seen = 0, cases = 0;
    for ( int round = 0; round < 400; ++round )
    {
        TokenAutomaton a;
        const int V = 1 + below( 40 );
        a.num_states = 1 + below( 6 );
        // every other round each token is a class of its own; about 1.5 classes of a state have a transition, so that forced states are common
        const bool own = round % 2 == 0;
        a.num_classes = own ? V : 1 + below( std::min( V, 7 ) );
        a.class_of.resize( static_cast<size_t>( V ) );
        for ( size_t i = 0; i < a.class_of.size(); ++i ) a.class_of[ i ] = static_cast<uint16_t>( own ? static_cast<int>( i ) : below( a.num_classes ) );
        a.next.resize( static_cast<size_t>( a.num_states ) * a.num_classes );
        for ( auto& n : a.next ) n = below( 2 * a.num_classes ) >= 3 ? F : static_cast<uint16_t>( below( a.num_states ) );
        a.validate( V );
        // without a bias
        TokenBiasPlan none;
        const auto f0 = a.forcedTokens( none );
        expect( f0 == bruteForce( a, none ), "forcedTokens without a bias is the brute-force answer" );
        // with bans (never all tokens: composeTokenBias refuses a table without a finite entry)
        TokenBiasRequest rq;
        for ( int32_t t = 0; t < V; ++t ) if ( below( 3 ) == 0 && static_cast<int>( rq.banned_tokens.size() ) + 1 < V ) rq.banned_tokens.push_back( t );
        const TokenBiasPlan banned = composeTokenBias( rq, V );
        const auto f1 = a.forcedTokens( banned );
        expect( f1 == bruteForce( a, banned ), "forcedTokens with bans is the brute-force answer" );
        // an allow-list (fill -inf) with a bias and a ban inside it
        TokenBiasRequest al;
        for ( int32_t t = 0; t < V; ++t ) if ( below( 2 ) == 0 ) al.allowed_tokens.push_back( t );
        if ( al.allowed_tokens.empty() ) al.allowed_tokens.push_back( below( V ) );
        al.logit_bias.emplace_back( al.allowed_tokens.front(), 1.5f );
        if ( al.allowed_tokens.size() > 1 ) al.banned_tokens.push_back( al.allowed_tokens.back() );
        const TokenBiasPlan allowed = composeTokenBias( al, V );
        expect( a.forcedTokens( allowed ) == bruteForce( a, allowed ), "forcedTokens under an allow-list is the brute-force answer" );
        // min_tokens: the plan's initial table holds the stop tokens at -inf
        if ( V > 1 )
        {
            TokenBiasRequest mt;
            mt.min_tokens = 2;
            mt.stop_tokens = { static_cast<int32_t>( below( V ) ) };
            const TokenBiasPlan held = composeTokenBias( mt, V );
            expect( a.forcedTokens( held ) == bruteForce( a, held ), "forcedTokens before a min_tokens restore is the brute-force answer" );
        }
        for ( int32_t f : f0 ) forced_seen += f >= 0;
        for ( int32_t f : f1 ) forced_seen += f >= 0;
        cases += 2;
    }
    expect( forced_seen > 200, "the random automata have forced states" );

    // a state that is forced ONLY because of a ban: state 1 allows class 1 = tokens 6 and 7; state 2 allows class 0 = six tokens; state 0 allows everything
    TokenAutomaton a;
    a.num_states = 3; a.num_classes = 2; a.start = 0;
    a.class_of = { 0, 0, 0, 0, 0, 0, 1, 1 };
    a.next = { 0, 1, F, 2, 2, F };
    a.validate( 8 );
    TokenBiasPlan none;
    expect( a.forcedTokens( none ) == std::vector<int32_t>( { -1, -1, -1 } ), "no state of the hand-made automaton is forced without a bias" );
    TokenBiasRequest rq;
    rq.banned_tokens = { 6 };
    expect( a.forcedTokens( composeTokenBias( rq, 8 ) ) == std::vector<int32_t>( { -1, 7, -1 } ), "token 6 banned: state 1 is forced to token 7" );
    rq.banned_tokens = { 7, 0, 1, 2, 4, 5 };
    expect( a.forcedTokens( composeTokenBias( rq, 8 ) ) == std::vector<int32_t>( { -1, 6, 3 } ), "bans leave token 6 in state 1 and token 3 in state 2; state 0 keeps two" );
    rq.banned_tokens = { 6, 7 };
    expect( a.forcedTokens( composeTokenBias( rq, 8 ) ) == std::vector<int32_t>( { -1, -1, -1 } ), "a state left without a token is not forced" );
    if ( !bad ) std::printf( "token automaton forced OK (%d cases)\n", cases );
    return bad;
}
