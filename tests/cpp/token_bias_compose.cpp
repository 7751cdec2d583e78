// Mila/TokenBias.h, host only: the composition of logit_bias / banned_tokens / allowed_tokens / min_tokens into one bias table, its restore list and index, and every
// std::invalid_argument.  Compiled with g++ against the host include directory and run by tests/test_sample_biased_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>

#include "Mila/TokenBias.h"

using namespace Mila::Dnn;

static int failures = 0;
#define CHECK( cond ) do { if ( !( cond ) ) { std::printf( "FAILED line %d: %s\n", __LINE__, #cond ); ++failures; } } while ( 0 )

static const float NINF = -std::numeric_limits<float>::infinity();
constexpr int64_t V = 100;

// the dense table a plan describes
static std::vector<float> dense( const TokenBiasPlan& p )
{
    std::vector<float> t( V, p.fill );
    for ( size_t i = 0; i < p.ids.size(); ++i ) t[ static_cast<size_t>( p.ids[ i ] ) ] = p.values[ i ];
    return t;
}
static std::vector<float> restored( const TokenBiasPlan& p )
{
    std::vector<float> t = dense( p );
    for ( size_t i = 0; i < p.restore_ids.size(); ++i ) t[ static_cast<size_t>( p.restore_ids[ i ] ) ] = p.restore_values[ i ];
    return t;
}
static bool wellFormed( const TokenBiasPlan& p )
{
    if ( p.ids.size() != p.values.size() || p.restore_ids.size() != p.restore_values.size() ) return false;
    for ( size_t i = 1; i < p.ids.size(); ++i ) if ( p.ids[ i - 1 ] >= p.ids[ i ] ) return false;
    for ( size_t i = 1; i < p.restore_ids.size(); ++i ) if ( p.restore_ids[ i - 1 ] >= p.restore_ids[ i ] ) return false;
    for ( float v : p.values ) if ( std::isnan( v ) || v == -NINF ) return false;
    return true;
}
template<typename F> static bool refuses( F&& f )
{
    try { f(); } catch ( const std::invalid_argument& ) { return true; } catch ( ... ) { return false; }
    return false;
}

int main()
{
    {   // nothing set: no table at all
        TokenBiasRequest rq;
        rq.stop_tokens = { 1 };
        const TokenBiasPlan p = composeTokenBias( rq, V );
        CHECK( !p.active && p.ids.empty() && !p.hasRestore() && !rq.any() );
    }
    {   // logit_bias alone
        TokenBiasRequest rq;
        rq.logit_bias = { { 7, 2.5f }, { 3, -4.0f }, { 99, 100.0f } };
        const TokenBiasPlan p = composeTokenBias( rq, V );
        CHECK( p.active && wellFormed( p ) && p.fill == 0.0f && !p.hasRestore() );
        const auto t = dense( p );
        CHECK( t[ 7 ] == 2.5f && t[ 3 ] == -4.0f && t[ 99 ] == 100.0f && t[ 0 ] == 0.0f && t[ 50 ] == 0.0f );
        CHECK( p.ids == ( std::vector<int32_t>{ 3, 7, 99 } ) );
    }
    {   // a ban alone (a repeated id is fine)
        TokenBiasRequest rq;
        rq.banned_tokens = { 5, 0, 5 };
        const TokenBiasPlan p = composeTokenBias( rq, V );
        const auto t = dense( p );
        CHECK( p.active && wellFormed( p ) && p.fill == 0.0f && t[ 5 ] == NINF && t[ 0 ] == NINF && t[ 1 ] == 0.0f && p.ids.size() == 2 );
    }
    {   // an allow-list alone: everything else is forbidden, the allowed ids are 0
        TokenBiasRequest rq;
        rq.allowed_tokens = { 10, 20, 30 };
        const TokenBiasPlan p = composeTokenBias( rq, V );
        const auto t = dense( p );
        CHECK( p.active && wellFormed( p ) && p.fill == NINF );
        int finite = 0;
        for ( float v : t ) finite += std::isfinite( v ) ? 1 : 0;
        CHECK( finite == 3 && t[ 10 ] == 0.0f && t[ 20 ] == 0.0f && t[ 30 ] == 0.0f );
    }
    {   // min_tokens alone: the stop ids are forbidden at first, and come back with the value of the table without min_tokens (0)
        TokenBiasRequest rq;
        rq.stop_tokens = { 2, 1, 2 };
        rq.min_tokens = 6;
        rq.max_new_tokens = 6;
        const TokenBiasPlan p = composeTokenBias( rq, V );
        const auto t = dense( p ), r = restored( p );
        CHECK( p.active && wellFormed( p ) && p.fill == 0.0f && t[ 1 ] == NINF && t[ 2 ] == NINF && t[ 3 ] == 0.0f );
        CHECK( p.restore_ids == ( std::vector<int32_t>{ 1, 2 } ) && p.restore_values == ( std::vector<float>{ 0.0f, 0.0f } ) && p.restore_index == 6 );
        for ( float v : r ) CHECK( v == 0.0f );
    }
    {   // all four: a ban wins over an allow, the allowed ids carry their bias, a logit_bias outside the allow-list stays forbidden, the restore brings back what the
        // table without min_tokens holds -- a banned stop token stays banned, an allowed one gets its bias, one outside the list -inf
        TokenBiasRequest rq;
        rq.logit_bias = { { 10, 1.5f }, { 40, 9.0f }, { 60, 100.0f } };
        rq.allowed_tokens = { 10, 20, 30, 60, 61 };
        rq.banned_tokens = { 20 };
        rq.stop_tokens = { 60, 61, 62, 20 };
        rq.min_tokens = 3;
        const TokenBiasPlan p = composeTokenBias( rq, V );
        CHECK( p.active && wellFormed( p ) && p.fill == NINF && p.restore_index == 3 );
        const auto t = dense( p ), r = restored( p );
        CHECK( t[ 10 ] == 1.5f && t[ 30 ] == 0.0f && t[ 20 ] == NINF && t[ 40 ] == NINF && t[ 60 ] == NINF && t[ 61 ] == NINF && t[ 62 ] == NINF );
        CHECK( p.restore_ids == ( std::vector<int32_t>{ 20, 60, 61, 62 } ) );
        CHECK( r[ 60 ] == 100.0f && r[ 61 ] == 0.0f && r[ 62 ] == NINF && r[ 20 ] == NINF && r[ 10 ] == 1.5f && r[ 40 ] == NINF );
        // the restored table is the composition without min_tokens
        TokenBiasRequest no_min = rq;
        no_min.min_tokens = 0;
        const TokenBiasPlan q = composeTokenBias( no_min, V );
        CHECK( !q.hasRestore() && dense( q ) == r );
    }
    {   // min_tokens = 0 holds nothing back; without a stop set there is nothing to hold
        TokenBiasRequest rq;
        rq.logit_bias = { { 4, 100.0f } };
        rq.stop_tokens = { 4 };
        const TokenBiasPlan p = composeTokenBias( rq, V );
        CHECK( !p.hasRestore() && dense( p )[ 4 ] == 100.0f );
        TokenBiasRequest only_min;
        only_min.min_tokens = 2;
        CHECK( !composeTokenBias( only_min, V ).active );
    }
    // every invalid_argument
    auto with = []( auto&& edit ) { TokenBiasRequest rq; edit( rq ); return rq; };
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.logit_bias = { { -1, 1.0f } }; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.logit_bias = { { (int32_t)V, 1.0f } }; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.banned_tokens = { (int32_t)V }; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.allowed_tokens = { 1, -3 }; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.stop_tokens = { 1000 }; r.min_tokens = 1; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.logit_bias = { { 1, std::nanf( "" ) } }; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.logit_bias = { { 1, -NINF } }; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.logit_bias = { { 1, NINF } }; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.logit_bias = { { 1, 1.0f }, { 2, 1.0f }, { 1, 2.0f } }; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.allowed_tokens = { 5, 6 }; r.banned_tokens = { 6, 5 }; } ), V ); } ) );                       // nothing left
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.banned_tokens = { 0, 1, 2 }; } ), 3 ); } ) );                                                  // the whole vocabulary
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.allowed_tokens = { 5, 6 }; r.stop_tokens = { 5, 6 }; r.min_tokens = 1; } ), V ); } ) );        // nothing left before the restore
    CHECK( !refuses( [&] { composeTokenBias( with( []( auto& r ) { r.allowed_tokens = { 5, 6 }; r.stop_tokens = { 5, 6 }; r.min_tokens = 0; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.min_tokens = -1; } ), V ); } ) );
    CHECK( refuses( [&] { composeTokenBias( with( []( auto& r ) { r.min_tokens = 5; r.max_new_tokens = 4; } ), V ); } ) );
    CHECK( !refuses( [&] { composeTokenBias( with( []( auto& r ) { r.min_tokens = 5; r.max_new_tokens = 5; r.stop_tokens = { 1 }; } ), V ); } ) );
    CHECK( !refuses( [&] { composeTokenBias( with( []( auto& r ) { r.min_tokens = 500; r.stop_tokens = { 1 }; } ), V ); } ) );                                      // no budget set
    CHECK( refuses( [&] { composeTokenBias( TokenBiasRequest{}, 0 ); } ) );
    if ( failures ) { std::printf( "%d check(s) failed\n", failures ); return 1; }
    std::printf( "token bias compose OK\n" );
    return 0;
}
