// Host-only facts of row requests (compiled AND run, without a GPU, by tests/test_row_requests_cpu.py with the host flags of mila_amd/build.py): the per-row request
// checks of GemmaModel::generateRequests (Mila/GemmaModel.h: planRowRequest) with the row's number in every message, the per-row bias plans and restore indices, the
// layout of the device records, and the surface on the transformer and the model.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

#include "Mila/GemmaModel.h"

using namespace Mila::Dnn;

static_assert( sizeof( mila_sample_row_params ) == 32 && offsetof( mila_sample_row_params, temperature ) == 0 && offsetof( mila_sample_row_params, top_k ) == 4 &&
               offsetof( mila_sample_row_params, top_p ) == 8 && offsetof( mila_sample_row_params, min_p ) == 12 && offsetof( mila_sample_row_params, repetition_penalty ) == 16 &&
               offsetof( mila_sample_row_params, inv_rep ) == 20 && offsetof( mila_sample_row_params, presence_penalty ) == 24 &&
               offsetof( mila_sample_row_params, frequency_penalty ) == 28 );
static_assert( sizeof( mila_token_automaton_row ) == 24 && offsetof( mila_token_automaton_row, next ) == 8 && offsetof( mila_token_automaton_row, S ) == 16 &&
               offsetof( mila_token_automaton_row, C ) == 20 );

template<typename Net>
concept RowRequestsSurface = requires( Net& n, std::span<const typename Net::SamplingParams> rq, const float* draws, const int32_t* ids, const float* values, const TokenAutomaton& a )
{
    n.setRowsRequests( rq, draws );
    n.clearRowsRequests();
    { n.rowsRequestsOn() } -> std::same_as<bool>;
    n.setRowTokenBias( 0, 0.0f, ids, values, size_t( 0 ) );
    n.clearRowTokenBias( 0 );
    n.stageRowTokenBiasUpdate( 0, ids, values, size_t( 0 ) );
    n.commitRowTokenBiasUpdate( 0 );
    n.setRowTokenAutomaton( 0, a );
    n.clearRowTokenAutomaton( 0 );
    { n.rowTokenAutomatonState( 0 ) } -> std::same_as<std::optional<int32_t>>;
    n.sampleRowRequest( 0, 0.5f );
};
static_assert( RowRequestsSurface<GemmaTransformer<Quant::Weight::NoWeightQuant>> && RowRequestsSurface<GemmaTransformer<Quant::Weight::PerChannelFp8<>>> &&
               RowRequestsSurface<GemmaTransformer<Quant::Weight::PerGroupFp4<128>>> );

constexpr dim_t V = 100, CONTEXT = 64;
static const std::unordered_set<int32_t> STOPS{ 1, 2 };
static int failures = 0;
#define CHECK( cond ) do { if ( !( cond ) ) { std::printf( "FAILED line %d: %s\n", __LINE__, #cond ); ++failures; } } while ( 0 )

static BatchRequest request()
{
    BatchRequest r;
    r.prompt = { 5, 6, 7 };
    r.seed = 9;
    return r;
}
// the message of the refusal, "" when the request is accepted
template<typename F> static std::string refusal( F&& edit, int row = 2, std::optional<int> logprobs = std::nullopt )
{
    BatchRequest r = request();
    edit( r );
    try { (void)planRowRequest( r, logprobs, row, V, CONTEXT, STOPS ); }
    catch ( const std::invalid_argument& e ) { return e.what(); }
    return "";
}
static bool refusedAtRow( const std::string& msg, int row ) { return msg.find( "row " + std::to_string( row ) + ":" ) != std::string::npos; }

int main()
{
    const float NINF = -std::numeric_limits<float>::infinity();
    {   // a greedy request (top_k == 1, generate()'s rule): the record's greedy class; the model's stop set, no table
        BatchRequest r = request();
        r.params.sampling.top_k = 1;
        const RowRequestPlan p = planRowRequest( r, std::nullopt, 0, V, CONTEXT, STOPS );
        CHECK( p.greedy && p.sampling.temperature == 0.0f && p.sampling.top_k == 0 && p.sampling.top_p == 1.0f );
        CHECK( p.stop_ids == STOPS && p.max_new == CONTEXT && !p.bias.active && !p.bias.hasRestore() );
    }
    {   // stochastic: the record carries the request's seven fields
        BatchRequest r = request();
        r.params.sampling.temperature = 0.7f; r.params.sampling.top_k = 5; r.params.sampling.top_p = 0.9f; r.params.sampling.min_p = 0.05f;
        r.params.sampling.repetition_penalty = 1.2f; r.params.sampling.presence_penalty = 0.3f; r.params.sampling.frequency_penalty = 0.2f;
        r.params.max_new_tokens = 4;
        const RowRequestPlan p = planRowRequest( r, std::nullopt, 1, V, CONTEXT, STOPS );
        CHECK( !p.greedy && p.sampling.temperature == 0.7f && p.sampling.top_k == 5 && p.sampling.top_p == 0.9f && p.sampling.min_p == 0.05f );
        CHECK( p.sampling.repetition_penalty == 1.2f && p.sampling.presence_penalty == 0.3f && p.sampling.frequency_penalty == 0.2f && p.max_new == 4 );
        r.params.sampling.temperature = 0.0f;      // greedy by temperature: the penalties stay in the record, the truncations go
        const RowRequestPlan g = planRowRequest( r, std::nullopt, 1, V, CONTEXT, STOPS );
        CHECK( g.greedy && g.sampling.top_k == 0 && g.sampling.top_p == 1.0f && g.sampling.repetition_penalty == 1.2f && g.sampling.penalized() );
    }
    {   // per-row bias plans and restore indices: two rows with their own stop sets and min_tokens
        BatchRequest a = request(), b = request();
        a.params.stop_tokens = { 10, 11 }; a.params.min_tokens = 3; a.params.logit_bias = { { 10, 2.0f } };
        b.params.stop_tokens = { 20 }; b.params.min_tokens = 5; b.params.max_new_tokens = 8; b.params.banned_tokens = { 30 };
        const RowRequestPlan pa = planRowRequest( a, std::nullopt, 0, V, CONTEXT, STOPS ), pb = planRowRequest( b, std::nullopt, 1, V, CONTEXT, STOPS );
        CHECK( pa.stop_ids == ( std::unordered_set<int32_t>{ 10, 11 } ) && pb.stop_ids == ( std::unordered_set<int32_t>{ 20 } ) );
        CHECK( pa.bias.active && pa.bias.hasRestore() && pa.bias.restore_index == 3 && pa.bias.restore_ids == ( std::vector<int32_t>{ 10, 11 } ) );
        CHECK( pa.bias.restore_values == ( std::vector<float>{ 2.0f, 0.0f } ) );
        CHECK( pb.bias.active && pb.bias.hasRestore() && pb.bias.restore_index == 5 && pb.bias.restore_ids == ( std::vector<int32_t>{ 20 } ) );
        bool banned = false;
        for ( size_t i = 0; i < pb.bias.ids.size(); ++i ) banned = banned || ( pb.bias.ids[ i ] == 30 && pb.bias.values[ i ] == NINF );
        CHECK( banned );
    }
    {   // logprobs: one n for the call
        CHECK( refusal( []( auto& ) {}, 2, 3 ).find( "logprobs" ) != std::string::npos );
        CHECK( refusal( []( auto& r ) { r.params.logprobs = 3; }, 2, 3 ).empty() );
        CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.logprobs = 2; }, 1, 3 ), 1 ) );
        CHECK( !refusal( []( auto& r ) { r.params.logprobs = 21; }, 0, 21 ).empty() );
    }
    // every refusal names its row
    auto stochastic = []( BatchRequest& r ) { r.params.sampling.temperature = 0.8f; r.params.sampling.top_k = 0; };
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.prompt.clear(); } ), 2 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.prompt.assign( CONTEXT + 1, 3 ); } ), 2 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.prompt = { 1, (int32_t)V }; }, 3 ), 3 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.speculative_sampling = true; } ), 2 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.speculate_constrained = true; } ), 2 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.draft = []( std::span<const int32_t>, int ) { return std::vector<int32_t>{}; }; } ), 2 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.sampling.temperature = std::nanf( "" ); r.params.sampling.top_k = 0; } ), 2 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.sampling.repetition_penalty = 0.0f; } ), 2 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.sampling.min_p = 1.0f; } ), 2 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.sampling.presence_penalty = std::numeric_limits<float>::infinity(); } ), 2 ) );
    CHECK( refusedAtRow( refusal( [&]( auto& r ) { stochastic( r ); r.params.sampling.top_p = 0.0f; } ), 2 ) );
    CHECK( refusedAtRow( refusal( [&]( auto& r ) { stochastic( r ); r.params.sampling.top_k = -1; } ), 2 ) );
    CHECK( refusal( [&]( auto& r ) { stochastic( r ); } ).empty() );
    CHECK( refusal( []( auto& r ) { r.params.sampling.top_k = 1; r.params.sampling.top_p = 0.0f; } ).empty() );      // a greedy request: the truncations are not read
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.sampling.top_p = 0.0f; } ), 2 ) );                           // the default request is stochastic
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.logit_bias = { { (int32_t)V, 1.0f } }; } ), 2 ) );
    CHECK( refusedAtRow( refusal( []( auto& r ) { r.params.min_tokens = 5; r.params.max_new_tokens = 4; } ), 2 ) );
    {   // the reachability check is per row: an automaton whose second state allows nothing, and one that is live only until the row's bias bans its tokens
        auto dead = std::make_shared<TokenAutomaton>();
        dead->num_states = 2; dead->num_classes = 1; dead->start = 0;
        dead->class_of.assign( V, 0 );
        dead->next = { 1, TokenAutomaton::FORBIDDEN };
        CHECK( refusedAtRow( refusal( [&]( auto& r ) { r.params.automaton = dead; } ), 2 ) );
        auto live = std::make_shared<TokenAutomaton>();
        live->num_states = 2; live->num_classes = 2; live->start = 0;
        live->class_of.assign( V, 0 );
        for ( dim_t i = V / 2; i < V; ++i ) live->class_of[ static_cast<size_t>( i ) ] = 1;
        live->next = { 1, TokenAutomaton::FORBIDDEN, TokenAutomaton::FORBIDDEN, 0 };
        CHECK( refusal( [&]( auto& r ) { r.params.automaton = live; } ).empty() );
        CHECK( refusedAtRow( refusal( [&]( auto& r ) { r.params.automaton = live; for ( int32_t t = V / 2; t < V; ++t ) r.params.banned_tokens.push_back( t ); }, 1 ), 1 ) );
        CHECK( refusedAtRow( refusal( [&]( auto& r ) { r.params.automaton = live; r.params.min_tokens = 1; } ), 2 ) );
    }
    if ( failures ) { std::printf( "%d check(s) failed\n", failures ); return 1; }
    std::printf( "row requests compose OK\n" );
    return 0;
}
