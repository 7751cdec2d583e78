// Host-only facts of batched decode in the Gemma model (compiled AND run, without a GPU, by tests/test_decode_rows_cpu.py with the host flags of mila_amd/build.py):
// GemmaConfig::max_batch accepts 1 .. 4, and values above 1 are rejected together with kv_fp8 and with bounded_local_kv; the rows surface exists on the block
// interface and on the transformer.
#include <cstdio>
#include <stdexcept>

#include "Mila/GemmaModel.h"

using namespace Mila::Dnn;

template<typename L>
concept RowsCacheSurface = requires( L& l )
{
    l.setCacheRows( 2 );
    l.selectCacheRow( 1 );
    { l.keyCacheRows() } -> std::same_as<uint16_t*>;
    { l.valueCacheRows() } -> std::same_as<uint16_t*>;
};
static_assert( RowsCacheSurface<GemmaTransformer<Quant::Weight::NoWeightQuant>::Layer> );
static_assert( RowsCacheSurface<Compute::RocmGqaOpBase> );

template<typename Net>
concept RowsModelSurface = requires( Net& n, const typename Net::TokenTensor& t )
{
    n.prefillRow( 0, t, 1, 0 );
    n.resetRow( 0 );
    n.setRowActive( 0, true );
    n.decodeRows( 2, 0, true );
    n.ensureGraphRows( 2, 0, true );
    n.replayGraphRows();
    { n.graphRowsCaptureCount() } -> std::same_as<size_t>;
};
static_assert( RowsModelSurface<GemmaTransformer<Quant::Weight::NoWeightQuant>> && RowsModelSurface<GemmaTransformer<Quant::Weight::PerChannelFp8<>>> &&
               RowsModelSurface<GemmaTransformer<Quant::Weight::PerGroupFp4<128>>> );

static bool throwsInvalid( const GemmaConfig& c )
{
    try { c.validate(); }
    catch ( const std::invalid_argument& ) { return true; }
    return false;
}

int main()
{
    int bad = 0;
    auto expect = [&]( bool ok, const char* what ) { if ( !ok ) { std::printf( "FAILED: %s\n", what ); ++bad; } };
    GemmaConfig c;
    expect( c.max_batch == 1 && !throwsInvalid( c ), "the default is one sequence and valid" );
    for ( dim_t b : { 1, 2, 3, 4 } ) { c.max_batch = b; expect( !throwsInvalid( c ), "max_batch 1 .. 4 is accepted" ); }
    for ( dim_t b : { 0, 5, -1 } ) { c.max_batch = b; expect( throwsInvalid( c ), "max_batch 0, 5 and -1 throw" ); }
    c = GemmaConfig{}; c.max_batch = 2; c.kv_fp8 = true;
    expect( throwsInvalid( c ), "max_batch 2 with kv_fp8 throws" );
    c.max_batch = 1;
    expect( !throwsInvalid( c ), "kv_fp8 alone stays valid" );
    c = GemmaConfig{}; c.max_batch = 2; c.bounded_local_kv = true;
    expect( throwsInvalid( c ), "max_batch 2 with bounded_local_kv throws" );
    c.max_batch = 1;
    expect( !throwsInvalid( c ), "bounded_local_kv alone stays valid" );
    if ( !bad ) std::printf( "rows traits OK\n" );
    return bad;
}
