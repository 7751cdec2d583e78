// C entry points for ONE GroupedQueryAttention<Rocm, BF16, TKvPolicy> component of the host mirror, for the three KV-cache policies
// (Quantization/KvCache: NoKvCompression, SlidingWindowKvCache, PerChannelKvFp8<>): build, chunked prefill, decode, the device-position decode of the FP8 policy,
// rewind, state bytes and a read-back of the cache arrays (tests/test_kvfp8_host_gpu.py, tests/test_kvfp8_decode_at_host_gpu.py).  Errors go to the message mila_host_last_error() returns.
#include <cstring>
#include <memory>
#include <string>
#include <variant>

#include "Mila/GemmaBlock.h"

using namespace Mila::Dnn;

namespace Mila::Host { void setLastError( const std::string& text ); }      // gemma_runner.cpp

namespace
{
    using Plain = GroupedQueryAttention<DeviceType::Rocm, TensorDataType::BF16, Quant::KvCache::NoKvCompression>;
    using Ring = GroupedQueryAttention<DeviceType::Rocm, TensorDataType::BF16, Quant::KvCache::SlidingWindowKvCache>;
    using Fp8 = GroupedQueryAttention<DeviceType::Rocm, TensorDataType::BF16, Quant::KvCache::PerChannelKvFp8<>>;
    static_assert( std::is_same_v<Plain::OpType, Compute::RocmGqaOp<false>> && std::is_same_v<Ring::OpType, Compute::RocmGqaOp<true>> );
    static_assert( std::is_same_v<Fp8::OpType, Compute::RocmGqaKvFp8Op>, "PerChannelKvFp8<> must resolve to the FP8 KV cache op" );
    using TensorType = Tensor<TensorDataType::BF16, Compute::RocmDeviceMemoryResource>;

    struct GqaRunner
    {
        std::unique_ptr<Compute::IExecutionContext> ctx;
        std::variant<std::unique_ptr<Plain>, std::unique_ptr<Ring>, std::unique_ptr<Fp8>> gqa;
        dim_t B, NH, NKV, HS, max_seq, chunk;
        std::unique_ptr<TensorType> q, k, v;
        std::unique_ptr<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>> position;      ///< decodeAt's device position
    };
    template<typename F> int guarded( F&& f )
    {
        try { f(); return 0; }
        catch ( const std::invalid_argument& e ) { Mila::Host::setLastError( std::string( "invalid_argument: " ) + e.what() ); return MILA_E_INVALID_ARGUMENT; }
        catch ( const std::logic_error& e ) { Mila::Host::setLastError( std::string( "logic_error: " ) + e.what() ); return MILA_E_UNSUPPORTED; }
        catch ( const std::exception& e ) { Mila::Host::setLastError( e.what() ); return MILA_E_RUNTIME; }
    }
    template<typename G> std::unique_ptr<G> build( GqaRunner& r, const Compute::GqaOpConfig& c )
    {
        auto g = std::make_unique<G>( "gqa", GqaConfig( c.num_heads * c.head_dim, c.num_heads, c.num_kv_heads ).withWindow( c.window ).withAttentionScale( c.attention_scale ) );
        g->setExecutionContext( r.ctx.get() );
        g->build( BuildContext( shape_t{ r.B, r.max_seq, ( c.num_heads + 2 * c.num_kv_heads ) * c.head_dim }, RuntimeMode::Inference, false, r.chunk ) );
        return g;
    }
    Compute::ExecutionContext<DeviceType::Rocm>* rocm( GqaRunner* r ) { return Compute::cast_context<DeviceType::Rocm>( r->ctx.get() ); }
    /// host rows -> the runner's device tensor, as a [B, T, width] view
    TensorType upload( GqaRunner* r, TensorType& dst, const uint16_t* host, dim_t T, dim_t width )
    {
        Compute::rocmCheck( mila_cdna4_memcpy_h2d( dst.rawData(), host, static_cast<size_t>( r->B * T * width ) * 2, rocm( r )->getStream() ) );
        return dst.view( shape_t{ r->B, T, width } );
    }
}

extern "C" {
#define HOST_API __attribute__((visibility("default")))

/// Compute::GqaOpConfig as plain data
struct mila_gqa_op_config
{
    int64_t num_heads, num_kv_heads, head_dim, window;
    float attention_scale;      ///< <= 0 -> 1 / sqrt(head_dim)
};

/// kv_policy 0 NoKvCompression / 1 SlidingWindowKvCache / 2 PerChannelKvFp8<>; built (KV cache initialised) for `batch` sequences of up to max_seq tokens, prefill()
/// calls of up to prefill_chunk tokens (0 = max_seq)
HOST_API void* mila_gqa_create( int kv_policy, const mila_gqa_op_config* cfg, int64_t batch, int64_t max_seq, int64_t prefill_chunk, int device )
{
    GqaRunner* out = nullptr;
    int rc = guarded( [&]
    {
        if ( !cfg ) throw std::invalid_argument( "mila_gqa_create: null config" );
        if ( batch <= 0 || max_seq <= 0 || prefill_chunk < 0 ) throw std::invalid_argument( "mila_gqa_create: batch and max_seq must be positive" );
        if ( cfg->num_heads <= 0 || cfg->num_kv_heads <= 0 || cfg->head_dim <= 0 ) throw std::invalid_argument( "mila_gqa_create: head counts and head_dim must be positive" );
        const Compute::GqaOpConfig c{ cfg->num_heads, cfg->num_kv_heads, cfg->head_dim, cfg->window, cfg->attention_scale };
        auto r = std::make_unique<GqaRunner>();
        r->ctx = Compute::createExecutionContext( Compute::Device::Rocm( device ) );
        r->B = batch; r->NH = c.num_heads; r->NKV = c.num_kv_heads; r->HS = c.head_dim; r->max_seq = max_seq;
        r->chunk = prefill_chunk > 0 ? std::min( prefill_chunk, max_seq ) : max_seq;
        if ( kv_policy == 0 ) r->gqa = build<Plain>( *r, c );
        else if ( kv_policy == 1 ) r->gqa = build<Ring>( *r, c );
        else if ( kv_policy == 2 ) r->gqa = build<Fp8>( *r, c );
        else throw std::invalid_argument( "mila_gqa_create: kv_policy must be 0, 1 or 2" );
        r->q = std::make_unique<TensorType>( r->ctx->getDeviceId(), shape_t{ batch, r->chunk, c.num_heads * c.head_dim } );
        r->k = std::make_unique<TensorType>( r->ctx->getDeviceId(), shape_t{ batch, r->chunk, c.num_kv_heads * c.head_dim } );
        r->v = std::make_unique<TensorType>( r->ctx->getDeviceId(), shape_t{ batch, r->chunk, c.num_kv_heads * c.head_dim } );
        r->position = std::make_unique<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>>( r->ctx->getDeviceId(), shape_t{ 1 } );
        out = r.release();
    } );
    return rc == 0 ? out : nullptr;
}
HOST_API void mila_gqa_destroy( void* h ) { delete static_cast<GqaRunner*>( h ); }

/// IKvCacheLifecycle: an empty cache again
HOST_API int mila_gqa_init_cache( void* h )
{
    auto* r = static_cast<GqaRunner*>( h );
    return guarded( [&] { std::visit( [&]( auto& g ) { g->resetKVCache(); }, r->gqa ); } );
}

/// GroupedQueryAttention::prefill on host rows (bf16 bits): q [B, T, NH*HS], k / v [B, T, NKV*HS] at absolute positions position .. position + T - 1 -> y [B, T, NH*HS]
HOST_API int mila_gqa_prefill( void* h, const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t T, int64_t position, uint16_t* y )
{
    auto* r = static_cast<GqaRunner*>( h );
    return guarded( [&]
    {
        if ( T <= 0 || T > r->chunk ) throw std::invalid_argument( "mila_gqa_prefill: chunk outside (0, prefill_chunk]" );
        auto qv = upload( r, *r->q, q, T, r->NH * r->HS ), kv = upload( r, *r->k, k, T, r->NKV * r->HS ), vv = upload( r, *r->v, v, T, r->NKV * r->HS );
        std::visit( [&]( auto& g )
        {
            auto& out = g->prefill( qv, kv, vv, position );
            copyToHost( y, out, static_cast<size_t>( r->B * T * r->NH * r->HS ) * 2, rocm( r ) );
            rocm( r )->synchronize();
        }, r->gqa );
    } );
}

/// GroupedQueryAttention::decode: one token per sequence at absolute position `position`; q [B, NH*HS], k / v [B, NKV*HS] -> y [B, NH*HS]
HOST_API int mila_gqa_decode( void* h, const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t position, uint16_t* y )
{
    auto* r = static_cast<GqaRunner*>( h );
    return guarded( [&]
    {
        auto qv = upload( r, *r->q, q, 1, r->NH * r->HS ), kv = upload( r, *r->k, k, 1, r->NKV * r->HS ), vv = upload( r, *r->v, v, 1, r->NKV * r->HS );
        std::visit( [&]( auto& g )
        {
            auto& out = g->decode( qv, kv, vv, position );
            copyToHost( y, out, static_cast<size_t>( r->B * r->NH * r->HS ) * 2, rocm( r ) );
            rocm( r )->synchronize();
        }, r->gqa );
    } );
}

/// GroupedQueryAttention::decodeAt: the same step with the position in device memory (`position` is copied there first) and the live-length bound max_len; the
/// component's cache length is NOT advanced (mila_gqa_note_cache_length).  PerChannelKvFp8<> only: the bf16 policies answer MILA_E_UNSUPPORTED
HOST_API int mila_gqa_decode_at( void* h, const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t position, int64_t max_len, uint16_t* y )
{
    auto* r = static_cast<GqaRunner*>( h );
    return guarded( [&]
    {
        if ( position < 0 || position > INT32_MAX || max_len <= 0 || max_len > INT32_MAX ) throw std::invalid_argument( "mila_gqa_decode_at: position or max_len out of range" );
        auto qv = upload( r, *r->q, q, 1, r->NH * r->HS ), kv = upload( r, *r->k, k, 1, r->NKV * r->HS ), vv = upload( r, *r->v, v, 1, r->NKV * r->HS );
        const int32_t pos = static_cast<int32_t>( position );
        Compute::rocmCheck( mila_cdna4_memcpy_h2d( r->position->rawData(), &pos, sizeof( pos ), rocm( r )->getStream() ) );
        std::visit( [&]( auto& g )
        {
            if constexpr ( std::is_same_v<typename std::decay_t<decltype( *g )>::OpType, Compute::RocmGqaKvFp8Op> )
            {
                auto& out = g->decodeAt( qv, kv, vv, static_cast<const int32_t*>( r->position->rawData() ), max_len );
                copyToHost( y, out, static_cast<size_t>( r->B * r->NH * r->HS ) * 2, rocm( r ) );
                rocm( r )->synchronize();
            }
            else
                throw std::logic_error( "mila_gqa_decode_at: only the PerChannelKvFp8<> op has a device-position decode" );
        }, r->gqa );
    } );
}

/// the component's noteCacheLength( length ): what a caller of decodeAt reports once it knows the position
HOST_API int mila_gqa_note_cache_length( void* h, int64_t length )
{
    auto* r = static_cast<GqaRunner*>( h );
    return guarded( [&] { std::visit( [&]( auto& g ) { g->noteCacheLength( length ); }, r->gqa ); } );
}

/// the op's rewindKvCache( length ): throws where the component's bool-returning form would return false
HOST_API int mila_gqa_rewind( void* h, int64_t length )
{
    auto* r = static_cast<GqaRunner*>( h );
    return guarded( [&] { std::visit( [&]( auto& g ) { g->getOperation().rewindKvCache( length ); }, r->gqa ); } );
}

/// out[0] = the op's stateBytes(), out[1] = its requiredStateBytes( batch, max_seq, chunk ), out[2] = the component's getMemoryStats().device_state_bytes,
/// out[3] = its getRequiredMemory( build context ).device_state_bytes, out[4] = cacheCapacity(), out[5] = cacheLength()
HOST_API int mila_gqa_state_bytes( void* h, int64_t* out )
{
    auto* r = static_cast<GqaRunner*>( h );
    return guarded( [&]
    {
        std::visit( [&]( auto& g )
        {
            auto& op = g->getOperation();
            out[ 0 ] = static_cast<int64_t>( op.stateBytes() );
            out[ 1 ] = static_cast<int64_t>( op.requiredStateBytes( static_cast<int>( r->B ), r->max_seq, r->chunk ) );
            out[ 2 ] = static_cast<int64_t>( g->getMemoryStats().device_state_bytes );
            const BuildContext bc( shape_t{ r->B, r->max_seq, ( r->NH + 2 * r->NKV ) * r->HS }, RuntimeMode::Inference, false, r->chunk );
            out[ 3 ] = static_cast<int64_t>( g->getRequiredMemory( bc ).device_state_bytes );
            out[ 4 ] = g->cacheCapacity();
            out[ 5 ] = g->cacheLength();
        }, r->gqa );
    } );
}

/// the cache arrays back on the host.  PerChannelKvFp8<>: k8 / v8 [B, NKV, capacity, HS] bytes, ks / vs [B, NKV, capacity] floats.  The bf16 policies: k8 / v8 receive
/// the bf16 caches (2 bytes per element), ks / vs are not written.  NULL pointers are skipped.
HOST_API int mila_gqa_read_cache( void* h, void* k8, void* v8, float* ks, float* vs )
{
    auto* r = static_cast<GqaRunner*>( h );
    return guarded( [&]
    {
        auto* ctx = rocm( r );
        auto d2h = [&]( void* dst, const void* src, size_t bytes ) { if ( dst ) Compute::rocmCheck( mila_cdna4_memcpy_d2h( dst, src, bytes, ctx->getStream() ) ); };
        std::visit( [&]( auto& g )
        {
            auto& op = g->getOperation();
            const size_t rows = static_cast<size_t>( r->B * r->NKV * op.cacheCapacity() );
            if constexpr ( std::is_same_v<std::decay_t<decltype( op )>, Compute::RocmGqaKvFp8Op> )
            {
                d2h( k8, op.keyStorage()->rawData(), rows * r->HS );
                d2h( v8, op.valueStorage()->rawData(), rows * r->HS );
                d2h( ks, op.keyScales()->rawData(), rows * 4 );
                d2h( vs, op.valueScales()->rawData(), rows * 4 );
            }
            else
            {
                d2h( k8, op.keyCache(), rows * r->HS * 2 );
                d2h( v8, op.valueCache(), rows * r->HS * 2 );
            }
        }, r->gqa );
        ctx->synchronize();
    } );
}

/// the methods that exist for the fused q/k/v entries only: which = 0 prefillFromCache, 1 keyCache, 2 valueCache.  The bf16 policies return 0; PerChannelKvFp8<>
/// throws std::logic_error (MILA_E_UNSUPPORTED, the message in mila_host_last_error)
HOST_API int mila_gqa_fused_surface_probe( void* h, int which )
{
    auto* r = static_cast<GqaRunner*>( h );
    return guarded( [&]
    {
        std::visit( [&]( auto& g )
        {
            if ( which == 1 ) { (void)g->keyCache(); return; }
            if ( which == 2 ) { (void)g->valueCache(); return; }
            auto qv = r->q->view( shape_t{ r->B, 1, r->NH * r->HS } );
            TensorType out( r->ctx->getDeviceId(), shape_t{ r->B, 1, r->NH * r->HS } );
            if constexpr ( !std::is_same_v<typename std::decay_t<decltype( *g )>::OpType, Compute::RocmGqaKvFp8Op> )
                if ( g->cacheLength() < 1 ) throw std::runtime_error( "mila_gqa_fused_surface_probe: append a token first" );
            g->prefillFromCache( qv, out, 1, static_cast<int>( g->cacheLength() ) - 1 );
            rocm( r )->synchronize();
        }, r->gqa );
    } );
}
}
