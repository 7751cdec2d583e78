// Host-only facts of the ring rows model (compiled AND run, without a GPU, by tests/test_ring_rows_cpu.py with the host flags of mila_amd/build.py):
// GemmaConfig::bounded_local_kv_rows admits max_batch 1 .. 4 and implies nothing a one-row bounded_local_kv model does not have; plain bounded_local_kv keeps its refusal
// and its message; the switch is refused with the FP8 KV cache, with draft tokens and without a window; GemmaModelConfig carries it; the transformer and PrefixCache have
// the ring surface.
#include <cstdio>
#include <stdexcept>
#include <string>

#include "Mila/GemmaModel.h"

using namespace Mila::Dnn;

template<typename Net>
concept RingRowsSurface = requires( Net& n )
{
    { n.rowsRingCapacity() } -> std::same_as<dim_t>;
    { n.rewindKvCacheRow( 0, dim_t( 1 ), dim_t( 2 ) ) } -> std::same_as<bool>;
    n.forkRow( 0, 2u, dim_t( 1 ) );
    n.forkRowPrefix( 0, 2u, dim_t( 1 ) );
};
static_assert( RingRowsSurface<GemmaTransformer<Quant::Weight::NoWeightQuant>> && RingRowsSurface<GemmaTransformer<Quant::Weight::PerChannelFp8<>>> &&
               RingRowsSurface<GemmaTransformer<Quant::Weight::PerGroupFp4<128>>> );
static_assert( std::is_same_v<GemmaTransformer<Quant::Weight::NoWeightQuant>::BoundedLocalBlockType::AttentionType::OpType, Compute::RocmGqaOp<true>> );
static_assert( sizeof( mila_kv_fork_layer_band ) == 32 );

static std::string refusal( const GemmaConfig& c )
{
    try { c.validate(); }
    catch ( const std::invalid_argument& e ) { return e.what(); }
    return "";
}

int main()
{
    int bad = 0;
    auto expect = [&]( bool ok, const char* what ) { if ( !ok ) { std::printf( "FAILED: %s\n", what ); ++bad; } };
    auto has = []( const std::string& s, const char* part ) { return s.find( part ) != std::string::npos; };
    GemmaConfig c;
    expect( !c.bounded_local_kv_rows && !c.boundedLocalKv(), "the switch is off by default" );
    for ( dim_t b : { 1, 2, 3, 4 } ) { c = GemmaConfig{}; c.bounded_local_kv_rows = true; c.max_batch = b; expect( refusal( c ).empty() && c.boundedLocalKv(), "the switch admits max_batch 1 .. 4" ); }
    c = GemmaConfig{}; c.bounded_local_kv_rows = true; c.bounded_local_kv = true; c.max_batch = 3;
    expect( refusal( c ).empty(), "naming both switches is the same configuration" );
    c = GemmaConfig{}; c.bounded_local_kv = true; c.max_batch = 2;
    expect( has( refusal( c ), "max_batch > 1 cannot be combined with bounded_local_kv (the ring needs a rewind rule per row)" ), "plain bounded_local_kv keeps its refusal and its message" );
    c = GemmaConfig{}; c.bounded_local_kv_rows = true; c.kv_fp8 = true;
    expect( has( refusal( c ), "bounded_local_kv_rows cannot be combined with kv_fp8" ), "refused with kv_fp8" );
    c = GemmaConfig{}; c.bounded_local_kv_rows = true; c.kv_fp8_rows = true; c.max_batch = 2;
    expect( has( refusal( c ), "bounded_local_kv_rows cannot be combined with kv_fp8" ), "refused with kv_fp8_rows" );
    c = GemmaConfig{}; c.bounded_local_kv_rows = true; c.draft_tokens = 2;
    expect( has( refusal( c ), "bounded_local_kv_rows cannot be combined with draft_tokens > 0" ), "refused with draft tokens" );
    for ( dim_t w : { 0, -4 } ) { c = GemmaConfig{}; c.bounded_local_kv_rows = true; c.window = w; expect( has( refusal( c ), "bounded_local_kv_rows needs a sliding window" ), "refused without a window" ); }
    for ( dim_t b : { 0, 5 } ) { c = GemmaConfig{}; c.bounded_local_kv_rows = true; c.max_batch = b; expect( has( refusal( c ), "outside 1 .. 4" ), "max_batch stays 1 .. 4" ); }
    GemmaModelConfig mc( 64 );
    expect( !mc.boundedLocalKvRows() && mc.withBoundedLocalKvRows( true ).boundedLocalKvRows() && !mc.boundedLocalKv(), "GemmaModelConfig carries the switch beside withBoundedLocalKv" );
    PrefixCache flat( 4 ), ring( 4, 8, 11 );
    expect( flat.window() == 0 && flat.capacity() == 0 && ring.window() == 8 && ring.capacity() == 11, "PrefixCache takes the ring geometry, 0 / 0 by default" );
    if ( !bad ) std::printf( "ring rows traits OK\n" );
    return bad;
}
