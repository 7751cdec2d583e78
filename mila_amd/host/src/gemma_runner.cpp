// C entry points over the C++ host mirror for bench.py / tests (plain pointers and sizes only).
// Instantiates GemmaTransformer<TWeightQuant> for the three weight policies of BASELINE.json
// configs 3-5 and exposes build / prefill / decode / timing.
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <random>
#include <span>
#include <string>
#include <variant>

#include "Mila/GemmaModel.h"

using namespace Mila::Dnn;
using Quant::Weight::NoWeightQuant;
using Quant::Weight::PerChannelFp8;
using Quant::Weight::PerGroupFp4;

namespace
{
    thread_local std::string g_err;

    struct Runner
    {
        std::variant<std::unique_ptr<GemmaTransformer<NoWeightQuant>>, std::unique_ptr<GemmaTransformer<PerChannelFp8<>>>,
                     std::unique_ptr<GemmaTransformer<PerGroupFp4<128>>>> model;
        std::unique_ptr<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>> tokens;
        dim_t max_prefill{ 1 };
        // generate_sampled's graph mode: the draw ring the captured stochastic step reads, the token ring it publishes into, and the device sequence counter --
        // allocated at the first such call and kept, so that a later call with the same sampling parameters finds its capture still valid
        static constexpr int kRing = 8;
        float* draws_host{ nullptr };
        unsigned long long* ring_host{ nullptr };
        const float* draws_dev{ nullptr };
        unsigned long long* ring_dev{ nullptr };
        std::unique_ptr<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>> seq_dev;      // one 64-bit counter
        uint64_t samples{ 0 };                                                                       // its value
        // decode_rows / chain_decode with a sampler tail: one draw per row, host-visible, allocated at the first such call
        // the sampling filters of the step-level calls (mila_gemma_set_sampling_filters): min_p, repetition_penalty, presence_penalty, frequency_penalty
        float filters[ 4 ]{ 0.0f, 1.0f, 0.0f, 0.0f };
        template<typename TSp> void applyFilters( TSp& sp ) const
        {
            sp.min_p = filters[ 0 ]; sp.repetition_penalty = filters[ 1 ]; sp.presence_penalty = filters[ 2 ]; sp.frequency_penalty = filters[ 3 ];
        }
        static constexpr int kStepDraws = 4;
        float* step_draws_host{ nullptr };
        const float* step_draws_dev{ nullptr };
        /// the device address of the step draws, holding draws[ 0 .. n )
        const float* stepDraws( const float* draws, int n )
        {
            if ( !draws || n < 1 || n > kStepDraws ) throw std::invalid_argument( "a sampled step takes 1 .. 4 draws" );
            if ( !step_draws_host )
            {
                hipCheck( hipHostMalloc( reinterpret_cast<void**>( &step_draws_host ), kStepDraws * sizeof( float ), hipHostMallocMapped | hipHostMallocCoherent ), "hipHostMalloc (mapped, coherent step draws)" );
                void* dptr = nullptr;
                hipCheck( hipHostGetDevicePointer( &dptr, step_draws_host, 0 ), "hipHostGetDevicePointer" );
                step_draws_dev = static_cast<const float*>( dptr );
            }
            for ( int i = 0; i < kStepDraws; ++i )
            {
                const float v = i < n ? draws[ i ] : 0.0f;
                uint32_t bits;
                std::memcpy( &bits, &v, 4 );
                __atomic_store_n( reinterpret_cast<uint32_t*>( step_draws_host ) + i, bits, __ATOMIC_RELEASE );
            }
            return step_draws_dev;
        }
        ~Runner()
        {
            if ( step_draws_host ) (void)hipHostFree( step_draws_host );
            if ( draws_host ) (void)hipHostFree( draws_host );
            if ( ring_host ) (void)hipHostFree( ring_host );
        }
    };

    template<typename F> int guarded( F&& f )
    {
        try { f(); return 0; }
        catch ( const std::invalid_argument& e ) { g_err = std::string( "invalid_argument: " ) + e.what(); return MILA_E_INVALID_ARGUMENT; }
        catch ( const std::exception& e ) { g_err = e.what(); return MILA_E_RUNTIME; }
    }
}

// Gemma.Cuda.cpp:456-480 (KvPolicy_RoutesBoundedRingToLocalLayersOnly), the compile-time half: the sliding-window KV policy reaches the LOCAL block type only; global
// (full-attention) blocks are never bounded, whatever the policy.  (The byte footprint of the routing: tests/test_reference_scenarios_r4_gpu.py.)
namespace
{
    using ProbeNet = Mila::Dnn::GemmaTransformer<Mila::Dnn::Quant::Weight::NoWeightQuant>;
    static_assert( std::is_same_v<ProbeNet::BoundedLocalBlockType::AttentionType::OpType, Mila::Dnn::Compute::RocmGqaOp<true>>, "SlidingWindowKvCache must reach the local (sliding) layers" );
    static_assert( std::is_same_v<ProbeNet::LocalBlockType::AttentionType::OpType, Mila::Dnn::Compute::RocmGqaOp<false>>, "the default policy keeps local layers unbounded" );
    static_assert( std::is_same_v<ProbeNet::GlobalBlockType::AttentionType::OpType, Mila::Dnn::Compute::RocmGqaOp<false>>, "global (full-attention) layers must never be bounded" );
    static_assert( std::is_same_v<ProbeNet::KvFp8LocalBlockType::AttentionType::OpType, Mila::Dnn::Compute::RocmGqaKvFp8Op> &&
                   std::is_same_v<ProbeNet::KvFp8GlobalBlockType::AttentionType::OpType, Mila::Dnn::Compute::RocmGqaKvFp8Op>, "kv_fp8 puts the FP8 KV cache op on both kinds of layer" );
}

/// the other runners of this library (gqa_runner.cpp) report through the message mila_host_last_error() returns
namespace Mila::Host { void setLastError( const std::string& text ) { g_err = text; } }

extern "C" {

#define HOST_API __attribute__((visibility("default")))

struct mila_gemma_config
{
    int64_t vocab_size, embedding_dim, num_layers, num_heads, num_kv_heads, head_dim, hidden_dim, global_head_dim,
            num_global_kv_heads, window, sliding_window_pattern, global_rotary_dim;
    int64_t bounded_local_kv;   ///< != 0: SlidingWindowKvCache (ring of window + chunk - 1 rows) on the sliding-window layers
    int64_t kv_fp8;             ///< != 0: PerChannelKvFp8<> (e4m3 K / V + one fp32 scale per KV head per cached token) on every layer
};

HOST_API const char* mila_host_last_error( void ) { return g_err.c_str(); }

/// policy: 0 NoWeightQuant (bf16), 1 PerChannelFp8<>, 2 PerGroupFp4<128>.  cfg == NULL -> Gemma-4 12B.
/// device: HIP device ordinal of this replica (one process per GPU: the launcher's LOCAL_RANK)
HOST_API void* mila_gemma_create( int policy, const mila_gemma_config* c, int64_t max_seq, int64_t max_prefill, uint64_t seed, int device )
{
    Runner* r = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg;
        if ( c )
        {
            cfg.vocab_size = c->vocab_size; cfg.embedding_dim = c->embedding_dim; cfg.num_layers = c->num_layers; cfg.num_heads = c->num_heads;
            cfg.num_kv_heads = c->num_kv_heads; cfg.head_dim = c->head_dim; cfg.hidden_dim = c->hidden_dim; cfg.global_head_dim = c->global_head_dim;
            cfg.num_global_kv_heads = c->num_global_kv_heads; cfg.window = c->window; cfg.sliding_window_pattern = c->sliding_window_pattern;
            cfg.global_rotary_dim = c->global_rotary_dim;
            cfg.bounded_local_kv = c->bounded_local_kv != 0;
            cfg.kv_fp8 = c->kv_fp8 != 0;
        }
        auto rr = std::make_unique<Runner>();
        rr->max_prefill = max_prefill;
        switch ( policy )
        {
            case 0: rr->model = std::make_unique<GemmaTransformer<NoWeightQuant>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 1: rr->model = std::make_unique<GemmaTransformer<PerChannelFp8<>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 2: rr->model = std::make_unique<GemmaTransformer<PerGroupFp4<128>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            default: throw std::invalid_argument( "unknown weight policy" );
        }
        std::visit( [&]( auto& m )
        {
            m->initSynthetic( seed );
            rr->tokens = std::make_unique<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>>(
                m->context()->getDeviceId(), shape_t{ std::max<dim_t>( max_prefill, 1 ) } );
        }, rr->model );
        r = rr.release();
    } );
    return rc == 0 ? r : nullptr;
}

/// mila_gemma_create with GemmaConfig::max_batch: up to max_batch (1 .. 4) independent sequences per decode step.  mila_gemma_config itself is unchanged.
HOST_API void* mila_gemma_create_rows( int policy, const mila_gemma_config* c, int64_t max_seq, int64_t max_prefill, int64_t max_batch, uint64_t seed, int device )
{
    Runner* r = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg;
        if ( c )
        {
            cfg.vocab_size = c->vocab_size; cfg.embedding_dim = c->embedding_dim; cfg.num_layers = c->num_layers; cfg.num_heads = c->num_heads;
            cfg.num_kv_heads = c->num_kv_heads; cfg.head_dim = c->head_dim; cfg.hidden_dim = c->hidden_dim; cfg.global_head_dim = c->global_head_dim;
            cfg.num_global_kv_heads = c->num_global_kv_heads; cfg.window = c->window; cfg.sliding_window_pattern = c->sliding_window_pattern;
            cfg.global_rotary_dim = c->global_rotary_dim;
            cfg.bounded_local_kv = c->bounded_local_kv != 0;
            cfg.kv_fp8 = c->kv_fp8 != 0;
        }
        cfg.max_batch = max_batch;
        auto rr = std::make_unique<Runner>();
        rr->max_prefill = max_prefill;
        switch ( policy )
        {
            case 0: rr->model = std::make_unique<GemmaTransformer<NoWeightQuant>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 1: rr->model = std::make_unique<GemmaTransformer<PerChannelFp8<>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 2: rr->model = std::make_unique<GemmaTransformer<PerGroupFp4<128>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            default: throw std::invalid_argument( "unknown weight policy" );
        }
        std::visit( [&]( auto& m )
        {
            m->initSynthetic( seed );
            rr->tokens = std::make_unique<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>>(
                m->context()->getDeviceId(), shape_t{ std::max<dim_t>( max_prefill, 1 ) } );
        }, rr->model );
        r = rr.release();
    } );
    return rc == 0 ? r : nullptr;
}

static GemmaConfig gemma_config_of( const mila_gemma_config* c )
{
    GemmaConfig cfg;
    if ( c )
    {
        cfg.vocab_size = c->vocab_size; cfg.embedding_dim = c->embedding_dim; cfg.num_layers = c->num_layers; cfg.num_heads = c->num_heads;
        cfg.num_kv_heads = c->num_kv_heads; cfg.head_dim = c->head_dim; cfg.hidden_dim = c->hidden_dim; cfg.global_head_dim = c->global_head_dim;
        cfg.num_global_kv_heads = c->num_global_kv_heads; cfg.window = c->window; cfg.sliding_window_pattern = c->sliding_window_pattern;
        cfg.global_rotary_dim = c->global_rotary_dim;
        cfg.bounded_local_kv = c->bounded_local_kv != 0;
        cfg.kv_fp8 = c->kv_fp8 != 0;
    }
    return cfg;
}

/// mila_gemma_create with GemmaConfig::max_batch AND GemmaConfig::draft_tokens (0 .. 3: the chain step, chain_decode).  max_batch = 1 and draft_tokens = 0 build the
/// model mila_gemma_create builds.  mila_gemma_config itself is unchanged.
HOST_API void* mila_gemma_create_chain( int policy, const mila_gemma_config* c, int64_t max_seq, int64_t max_prefill, int64_t max_batch, int64_t draft_tokens, uint64_t seed, int device )
{
    Runner* r = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg = gemma_config_of( c );
        cfg.max_batch = max_batch;
        cfg.draft_tokens = draft_tokens;
        auto rr = std::make_unique<Runner>();
        rr->max_prefill = max_prefill;
        switch ( policy )
        {
            case 0: rr->model = std::make_unique<GemmaTransformer<NoWeightQuant>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 1: rr->model = std::make_unique<GemmaTransformer<PerChannelFp8<>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 2: rr->model = std::make_unique<GemmaTransformer<PerGroupFp4<128>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            default: throw std::invalid_argument( "unknown weight policy" );
        }
        std::visit( [&]( auto& m )
        {
            m->initSynthetic( seed );
            rr->tokens = std::make_unique<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>>(
                m->context()->getDeviceId(), shape_t{ std::max<dim_t>( max_prefill, 1 ) } );
        }, rr->model );
        r = rr.release();
    } );
    return rc == 0 ? r : nullptr;
}
/// GemmaConfig::validate() on the configuration mila_gemma_create_chain would build, without a device: 0, or MILA_E_INVALID_ARGUMENT and the message
HOST_API int mila_gemma_validate_config( const mila_gemma_config* c, int64_t max_batch, int64_t draft_tokens )
{
    return guarded( [&] { GemmaConfig cfg = gemma_config_of( c ); cfg.max_batch = max_batch; cfg.draft_tokens = draft_tokens; cfg.validate(); } );
}
/// ... with GemmaConfig::kv_fp8_rows (kv_fp8_rows != 0): the FP8 KV cache that max_batch > 1 may be combined with.  mila_gemma_config itself is unchanged.
HOST_API int mila_gemma_validate_config_kv( const mila_gemma_config* c, int64_t max_batch, int64_t draft_tokens, int kv_fp8_rows )
{
    return guarded( [&] { GemmaConfig cfg = gemma_config_of( c ); cfg.max_batch = max_batch; cfg.draft_tokens = draft_tokens; cfg.kv_fp8_rows = kv_fp8_rows != 0; cfg.validate(); } );
}
/// ... with GemmaConfig::bounded_local_kv_rows as well (bounded_local_kv_rows != 0): the rings that max_batch > 1 may be combined with
HOST_API int mila_gemma_validate_config_ring( const mila_gemma_config* c, int64_t max_batch, int64_t draft_tokens, int kv_fp8_rows, int bounded_local_kv_rows )
{
    return guarded( [&]
    {
        GemmaConfig cfg = gemma_config_of( c );
        cfg.max_batch = max_batch; cfg.draft_tokens = draft_tokens; cfg.kv_fp8_rows = kv_fp8_rows != 0; cfg.bounded_local_kv_rows = bounded_local_kv_rows != 0;
        cfg.validate();
    } );
}
/// mila_gemma_create_rows with GemmaConfig::bounded_local_kv_rows: max_batch (1 .. 4) sequences per decode step, each with its own rings on the sliding-window layers.
/// bounded_local_kv_rows = 0 builds the model mila_gemma_create_rows builds.
HOST_API void* mila_gemma_create_rows_ring( int policy, const mila_gemma_config* c, int64_t max_seq, int64_t max_prefill, int64_t max_batch, int bounded_local_kv_rows, uint64_t seed, int device )
{
    Runner* r = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg = gemma_config_of( c );
        cfg.max_batch = max_batch;
        cfg.bounded_local_kv_rows = bounded_local_kv_rows != 0;
        auto rr = std::make_unique<Runner>();
        rr->max_prefill = max_prefill;
        switch ( policy )
        {
            case 0: rr->model = std::make_unique<GemmaTransformer<NoWeightQuant>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 1: rr->model = std::make_unique<GemmaTransformer<PerChannelFp8<>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 2: rr->model = std::make_unique<GemmaTransformer<PerGroupFp4<128>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            default: throw std::invalid_argument( "unknown weight policy" );
        }
        std::visit( [&]( auto& m )
        {
            m->initSynthetic( seed );
            rr->tokens = std::make_unique<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>>(
                m->context()->getDeviceId(), shape_t{ std::max<dim_t>( max_prefill, 1 ) } );
        }, rr->model );
        r = rr.release();
    } );
    return rc == 0 ? r : nullptr;
}
/// mila_gemma_create_rows with GemmaConfig::kv_fp8_rows: max_batch (1 .. 4) sequences per decode step, each on its own FP8 KV caches.  kv_fp8_rows = 0 builds the model
/// mila_gemma_create_rows builds.
HOST_API void* mila_gemma_create_rows_kv( int policy, const mila_gemma_config* c, int64_t max_seq, int64_t max_prefill, int64_t max_batch, int kv_fp8_rows, uint64_t seed, int device )
{
    Runner* r = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg = gemma_config_of( c );
        cfg.max_batch = max_batch;
        cfg.kv_fp8_rows = kv_fp8_rows != 0;
        auto rr = std::make_unique<Runner>();
        rr->max_prefill = max_prefill;
        switch ( policy )
        {
            case 0: rr->model = std::make_unique<GemmaTransformer<NoWeightQuant>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 1: rr->model = std::make_unique<GemmaTransformer<PerChannelFp8<>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            case 2: rr->model = std::make_unique<GemmaTransformer<PerGroupFp4<128>>>( cfg, max_seq, max_prefill, Compute::Device::Rocm( device ) ); break;
            default: throw std::invalid_argument( "unknown weight policy" );
        }
        std::visit( [&]( auto& m )
        {
            m->initSynthetic( seed );
            rr->tokens = std::make_unique<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>>(
                m->context()->getDeviceId(), shape_t{ std::max<dim_t>( max_prefill, 1 ) } );
        }, rr->model );
        r = rr.release();
    } );
    return rc == 0 ? r : nullptr;
}
/// promptLookupDraft (GemmaModel.h), the default drafter of the speculative generate(): up to k tokens into out, returns their number.  Pure host code.
HOST_API int mila_gemma_prompt_lookup_draft( const int32_t* history, int64_t n, int k, int32_t* out )
{
    if ( !history || !out || n < 0 ) return 0;
    const auto d = promptLookupDraft( std::span<const int32_t>( history, static_cast<size_t>( n ) ), k );
    for ( size_t i = 0; i < d.size(); ++i ) out[ i ] = d[ i ];
    return static_cast<int>( d.size() );
}

/// regenerate the synthetic parameters under a profile: p = { linear_gain, qk_norm_center, post_norm_center, layer_scalar, table_gain }
HOST_API int mila_gemma_init_synthetic( void* h, uint64_t seed, const float* p )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        if ( !p ) throw std::invalid_argument( "init_synthetic: null profile" );
        std::visit( [&]( auto& m )
        {
            typename std::remove_reference_t<decltype( *m )>::SyntheticProfile pr;
            pr.linear_gain = p[ 0 ]; pr.qk_norm_center = p[ 1 ]; pr.post_norm_center = p[ 2 ]; pr.layer_scalar = p[ 3 ]; pr.table_gain = p[ 4 ];
            m->initSynthetic( seed, pr );
        }, r->model );
    } );
}

HOST_API void mila_gemma_destroy( void* h ) { delete static_cast<Runner*>( h ); }

static void upload_tokens( Runner* r, const int32_t* host_tokens, int64_t n )
{
    std::visit( [&]( auto& m )
    {
        Compute::rocmCheck( mila_cdna4_memcpy_h2d( r->tokens->data(), host_tokens, static_cast<size_t>( n ) * 4, m->context()->getStream() ) );
        m->context()->synchronize();
    }, r->model );
}

static void download_logits( Runner* r, float* host_logits )
{
    if ( !host_logits ) return;
    std::visit( [&]( auto& m )
    {
        auto& lg = m->logits();
        Compute::rocmCheck( mila_cdna4_memcpy_d2h( host_logits, lg.data(), lg.sizeInBytes(), m->context()->getStream() ) );
        m->context()->synchronize();
    }, r->model );
}

HOST_API int mila_gemma_prefill( void* h, const int32_t* host_tokens, int64_t T, int64_t position_offset, float* host_logits )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        if ( T <= 0 || T > r->max_prefill ) throw std::invalid_argument( "GemmaTransformer::prefill: chunk length out of range" );
        upload_tokens( r, host_tokens, T );
        std::visit( [&]( auto& m ) { m->prefill( *r->tokens, T, position_offset ); m->context()->synchronize(); }, r->model );
        download_logits( r, host_logits );
    } );
}

/// GemmaTransformer::prefillScored: mila_gemma_prefill that also scores rows [first_row, T) of the chunk.  host_targets[T]: the token whose log-probability row r
/// reports (the last row included; -1 = none: NaN).  out_logprob / out_argmax / out_argmax_logprob [T - first_row] (the two argmax outputs may both be NULL);
/// host_logits: the last row's logits as mila_gemma_prefill returns them (may be NULL)
HOST_API int mila_gemma_prefill_scored( void* h, const int32_t* host_tokens, int64_t T, int64_t position_offset, const int32_t* host_targets, int64_t first_row,
                                        float* out_logprob, int32_t* out_argmax, float* out_argmax_logprob, float* host_logits )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        if ( T <= 0 || T > r->max_prefill ) throw std::invalid_argument( "GemmaTransformer::prefillScored: chunk length out of range" );
        if ( !host_targets || !out_logprob ) throw std::invalid_argument( "prefill_scored: targets and out_logprob are required" );
        if ( ( out_argmax == nullptr ) != ( out_argmax_logprob == nullptr ) ) throw std::invalid_argument( "prefill_scored: the two argmax outputs go together" );
        upload_tokens( r, host_tokens, T );
        std::visit( [&]( auto& m )
        {
            Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource> targets( m->context()->getDeviceId(), shape_t{ T } );
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( targets.rawData(), host_targets, static_cast<size_t>( T ) * 4, m->context()->getStream() ) );
            m->prefillScored( *r->tokens, T, position_offset, targets.data(), first_row, out_argmax != nullptr );
            m->scoreOp().read( T - first_row, out_logprob, out_argmax, out_argmax_logprob );
        }, r->model );
        download_logits( r, host_logits );
    } );
}

/// on != 0 (default): prefill runs the fused glue kernels when the configuration fits; 0: one launch per reference op
HOST_API int mila_gemma_set_fused_prefill( void* h, int on )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { std::visit( [&]( auto& m ) { m->setFusedPrefill( on != 0 ); }, r->model ); } );
}
/// on != 0 (default): layers with a small split-partial set run the attention combine inside o_proj's prologue
/// GemmaTransformer::rewindKvCache( position ): *ok = 1 when every block accepted
HOST_API int mila_gemma_rewind( void* h, int64_t position, int* ok )
{
    return guarded( [&] { std::visit( [&]( auto& m ) { *ok = m->rewindKvCache( position ) ? 1 : 0; }, static_cast<Runner*>( h )->model ); } );
}

/// GemmaTransformer::prefillFrom( tokens[0 .. T), offset ): positions [0, offset) stay resident, the tail is prefilled; logits of the last position
HOST_API int mila_gemma_prefill_from( void* h, const int32_t* host_tokens, int64_t T, int64_t offset, float* host_logits )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            if ( T <= 0 ) throw std::invalid_argument( "prefill_from: empty prompt" );
            Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource> toks( m->context()->getDeviceId(), shape_t{ 1, T } );
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( toks.rawData(), host_tokens, static_cast<size_t>( T ) * 4, m->context()->getStream() ) );
            m->prefillFrom( toks, T, offset );
            m->context()->synchronize();
        }, r->model );
        download_logits( r, host_logits );
    } );
}

HOST_API int mila_gemma_set_prefill_overlap( void* h, int on )
{
    return guarded( [&] { std::visit( [&]( auto& m ) { m->setPrefillOverlap( on != 0 ); }, static_cast<Runner*>( h )->model ); } );
}

/// every parameter of the model in its storage form -> a SafeTensors file / back (component paths as tensor names)
HOST_API int mila_gemma_save_safetensors( void* h, const char* path )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { if ( !path ) throw std::invalid_argument( "save_safetensors: null path" ); std::visit( [&]( auto& m ) { m->saveSafeTensors( path ); }, r->model ); } );
}
HOST_API int mila_gemma_load_safetensors( void* h, const char* path )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { if ( !path ) throw std::invalid_argument( "load_safetensors: null path" ); std::visit( [&]( auto& m ) { m->loadSafeTensors( path ); }, r->model ); } );
}
/// the same tensors as a MILA .bin container / load from either container (sniffed by the leading magic, PretrainedReader.ixx:283-293)
HOST_API int mila_gemma_save_milabin( void* h, const char* path )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { if ( !path ) throw std::invalid_argument( "save_milabin: null path" ); std::visit( [&]( auto& m ) { m->saveMilaBin( path ); }, r->model ); } );
}
HOST_API int mila_gemma_load_pretrained( void* h, const char* path )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { if ( !path ) throw std::invalid_argument( "load_pretrained: null path" ); std::visit( [&]( auto& m ) { m->loadPretrained( path ); }, r->model ); } );
}
/// host-only (no device): list either container as the PretrainedModelReader sees it -- "name dtype nbytes d0,d1,.." lines in ascending
/// file-offset order, then "# container=mila|safetensors", "# mila_quantization=..", "# mila_config=<json>" lines
HOST_API int64_t mila_pretrained_list( const char* path, char* out, int64_t cap )
{
    int64_t need = -1;
    const int rc = guarded( [&]
    {
        Mila::Dnn::Serialization::PretrainedModelReader rd( path ? path : "" );
        std::string t;
        for ( auto& e : rd.entries() )
        {
            t += e.name + " " + e.dtype + " " + std::to_string( e.nbytes() ) + " ";
            for ( size_t d = 0; d < e.shape.size(); ++d ) t += ( d ? "," : "" ) + std::to_string( e.shape[ d ] );
            t += "\n";
        }
        t += std::string( "# container=" ) + ( rd.isMilaContainer() ? "mila" : "safetensors" ) + "\n";
        t += "# mila_quantization=" + rd.getWeightQuantization() + "\n";
        t += "# mila_config=" + rd.metadataJSON() + "\n";
        need = (int64_t)t.size();
        if ( out && cap > 0 ) { const size_t n = std::min<size_t>( t.size(), (size_t)cap - 1 ); std::memcpy( out, t.data(), n ); out[ n ] = 0; }
    } );
    return rc ? rc : need;
}
/// host-only: rewrite either container as a MILA .bin (tensor order = ascending source offsets); metadata_json == NULL keeps the source's
HOST_API int mila_pretrained_to_milabin( const char* src, const char* dst, const char* metadata_json )
{
    return guarded( [&]
    {
        Mila::Dnn::Serialization::PretrainedModelReader rd( src ? src : "" );
        Mila::Dnn::Serialization::MilaBinWriter wr( dst ? dst : "" );
        for ( auto& e : rd.entries() ) wr.declareTensor( e.name, e.dtype, e.shape );
        wr.setMetadataJSON( metadata_json ? std::string( metadata_json ) : rd.metadataJSON() );
        wr.beginData();
        for ( auto& e : rd.entries() ) wr.writeTensorData( e.name, e.data, e.nbytes() );
        wr.close();
    } );
}
/// host-only: the value the metadata parser extracts for `key` from a JSON text, round-tripped through toMetadataJSON (parser check)
HOST_API int64_t mila_pretrained_metadata_roundtrip( const char* json, char* out, int64_t cap )
{
    int64_t need = -1;
    const int rc = guarded( [&]
    {
        const std::string t = Mila::Dnn::Serialization::toMetadataJSON( Mila::Dnn::Serialization::parseMetadataJSON( json ? json : "" ) );
        need = (int64_t)t.size();
        if ( out && cap > 0 ) { const size_t n = std::min<size_t>( t.size(), (size_t)cap - 1 ); std::memcpy( out, t.data(), n ); out[ n ] = 0; }
    } );
    return rc ? rc : need;
}
/// host-only container checks (no device): list a file as "name dtype nbytes d0,d1,..\n" lines + "# key=value" metadata lines into out
/// (returns the length needed, or < 0 with mila_gemma_last_error set); copy src -> dst tensor by tensor through the reader and the writer
HOST_API int64_t mila_safetensors_list( const char* path, char* out, int64_t cap )
{
    int64_t need = -1;
    const int rc = guarded( [&]
    {
        Mila::Dnn::Serialization::SafeTensorsReader rd( path ? path : "" );
        std::string t;
        for ( auto& e : rd.entries() )
        {
            t += e.name + " " + e.dtype + " " + std::to_string( e.nbytes() ) + " ";
            for ( size_t d = 0; d < e.shape.size(); ++d ) t += ( d ? "," : "" ) + std::to_string( e.shape[ d ] );
            t += "\n";
        }
        for ( auto& [ k, v ] : rd.metadata() ) t += "# " + k + "=" + v + "\n";
        need = (int64_t)t.size();
        if ( out && cap > 0 ) { const size_t n = std::min<size_t>( t.size(), (size_t)cap - 1 ); std::memcpy( out, t.data(), n ); out[ n ] = 0; }
    } );
    return rc ? rc : need;
}
HOST_API int mila_safetensors_copy( const char* src, const char* dst )
{
    return guarded( [&]
    {
        Mila::Dnn::Serialization::SafeTensorsReader rd( src ? src : "" );
        Mila::Dnn::Serialization::SafeTensorsWriter wr( dst ? dst : "" );
        for ( auto& e : rd.entries() ) wr.declareTensor( e.name, e.dtype, e.shape );
        for ( auto& [ k, v ] : rd.metadata() ) wr.setMetadata( k, v );
        wr.beginData();
        for ( auto& e : rd.entries() ) wr.writeTensorData( e.name, e.data, e.nbytes() );
        wr.close();
    } );
}
/// on != 0 (default): quantized policies keep their prefill staging resident; 0: re-stage on every forward (the reference's way)
HOST_API int mila_gemma_set_resident_prefill_weights( void* h, int on )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { std::visit( [&]( auto& m ) { m->setResidentPrefillWeights( on != 0 ); }, r->model ); } );
}
/// fp4 policy: on != 0 (default, as in the reference) = W4A8 prefill on the fp8 matrix cores; 0 = dequantize -> bf16 GEMM
HOST_API int mila_gemma_set_fp8_activation_prefill( void* h, int on )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { std::visit( [&]( auto& m ) { m->setFp8ActivationPrefill( on != 0 ); }, r->model ); } );
}

/// mode: 0 reference-order (one launch per component), 1 fused schedule, 2 graph replay (position from device)
HOST_API int mila_gemma_decode( void* h, int32_t token, int64_t position, int mode, float* host_logits )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        upload_tokens( r, &token, 1 );
        std::visit( [&]( auto& m )
        {
            if ( mode == 0 ) m->decode( *r->tokens, position );
            else if ( mode == 1 ) m->decodeFused( *r->tokens, position );
            else
            {
                m->ensureGraph( *r->tokens, position );
                m->setDevicePosition( position );
                m->replayGraph();
            }
            m->context()->synchronize();
        }, r->model );
        download_logits( r, host_logits );
    } );
}

/// token log-probabilities in every step that follows, the timing loops among them (GemmaTransformer::setStepLogprobs, the device-output form): top_n = 0 .. 20, < 0 = off
HOST_API int mila_gemma_set_step_logprobs( void* h, int top_n )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m ) { if ( top_n < 0 ) m->setStepLogprobs( std::nullopt ); else m->setStepLogprobs( top_n ); }, static_cast<Runner*>( h )->model );
    } );
}
/// the outputs of the last step with log-probabilities: logprob [rows], ids / logprobs [rows * top_n]
static void read_logprobs( Runner* r, int rows, int top_n, float* out_logprob, int32_t* out_ids, float* out_logprobs )
{
    std::visit( [&]( auto& m ) { m->tokenLogprobs().read( rows, top_n, out_logprob, out_ids, out_logprobs ); }, r->model );
}
/// mila_gemma_decode, then the greedy sampler and the token's log-probabilities: *out_token = the greedy token of the step's logits, *out_logprob its log-probability,
/// out_ids / out_logprobs [top_n] the alternatives.  Modes 0 / 1 sample and report eagerly behind the step; mode 2 replays a graph captured with the greedy sampler
/// and the two log-probability nodes as its tail.  The setting is off again when the call returns (a later graph-mode step re-captures).
HOST_API int mila_gemma_decode_logprobs( void* h, int32_t token, int64_t position, int mode, int top_n, float* host_logits, int32_t* out_token, float* out_logprob,
                                         int32_t* out_ids, float* out_logprobs )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        upload_tokens( r, &token, 1 );
        std::visit( [&]( auto& m )
        {
            if ( top_n < 0 ) throw std::invalid_argument( "decode_logprobs: top_n must be 0 .. 20" );
            m->setStepLogprobs( top_n );
            const bool was = m->sampleInGraph();
            try
            {
                if ( mode == 0 ) { m->decode( *r->tokens, position ); m->sampleGreedy( *r->tokens ); m->enqueueStepLogprobs( r->tokens->data() ); }
                else if ( mode == 1 ) { m->decodeFused( *r->tokens, position ); m->sampleGreedy( *r->tokens ); m->enqueueStepLogprobs( r->tokens->data() ); }
                else
                {
                    m->setSampleInGraph( true );
                    m->ensureGraph( *r->tokens, position );
                    m->setDevicePosition( position );
                    m->replayGraph();
                }
                m->context()->synchronize();
            }
            catch ( ... ) { m->setSampleInGraph( was ); m->setStepLogprobs( std::nullopt ); throw; }
            m->setSampleInGraph( was );
            m->setStepLogprobs( std::nullopt );
            if ( out_token ) Compute::rocmCheck( mila_cdna4_memcpy_d2h( out_token, r->tokens->data(), 4, m->context()->getStream() ) );
            m->tokenLogprobs().read( 1, top_n, out_logprob, out_ids, out_logprobs );
        }, r->model );
        download_logits( r, host_logits );
    } );
}

/// Timed decode: `warmup` untimed steps then `steps` timed ones from `start_position`, token ids
/// cycling through a fixed pattern (the sampler is outside the measured path).

// ---- batched decode: rows of independent sequences (GemmaConfig::max_batch > 1) ------------------------------------------------------------------------
/// prefill T tokens at positions offset .. into row b's caches; host_logits (may be NULL): the last position's [vocab] logits
HOST_API int mila_gemma_prefill_row( void* h, int b, const int32_t* host_tokens, int64_t T, int64_t offset, float* host_logits )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            if ( T <= 0 ) throw std::invalid_argument( "prefill_row: empty prompt" );
            Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource> toks( m->context()->getDeviceId(), shape_t{ 1, T } );
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( toks.rawData(), host_tokens, static_cast<size_t>( T ) * 4, m->context()->getStream() ) );
            m->prefillRow( b, toks, T, offset );
            m->context()->synchronize();
        }, r->model );
        download_logits( r, host_logits );
    } );
}
/// row b's active word, and (token >= 0) the token its next step embeds
/// The sampling filters of the step-level calls that follow (filters[4] = min_p, repetition_penalty, presence_penalty, frequency_penalty; NULL = neutral): the greedy
/// samplers read them from the network (GemmaTransformer::setSamplingFilters), the stochastic ones get them with their SamplingParams (generate_sampled, decode_rows_sampled,
/// set_step_sampling for the rows step)
HOST_API int mila_gemma_set_sampling_filters( void* h, const float* filters )
{
    return guarded( [&]
    {
        auto* r = static_cast<Runner*>( h );
        const float neutral[ 4 ] = { 0.0f, 1.0f, 0.0f, 0.0f };
        const float* f = filters ? filters : neutral;
        std::visit( [&]( auto& m )
        {
            typename std::remove_reference_t<decltype( *m )>::SamplingParams sp;
            sp.min_p = f[ 0 ]; sp.repetition_penalty = f[ 1 ]; sp.presence_penalty = f[ 2 ]; sp.frequency_penalty = f[ 3 ];
            m->setSamplingFilters( sp );      // (validates; throws before the runner's copy changes)
        }, r->model );
        for ( int i = 0; i < 4; ++i ) r->filters[ i ] = f[ i ];
    } );
}
/// a new request on row `row` (0: the one-sequence interface): the token table cleared, the flags of the n prompt tokens set
HOST_API int mila_gemma_set_token_table( void* h, int row, const int32_t* prompt, int64_t n )
{
    return guarded( [&]
    {
        if ( n < 0 || ( n > 0 && !prompt ) ) throw std::invalid_argument( "set_token_table: null prompt" );
        std::visit( [&]( auto& m ) { m->resetTokenTable( row, prompt, static_cast<size_t>( n ) ); }, static_cast<Runner*>( h )->model );
    } );
}
/// row `row`'s table words [vocab] to the host
HOST_API int mila_gemma_read_token_table( void* h, int row, uint32_t* out )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            if ( !m->tokenTable() ) throw std::logic_error( "read_token_table: no token table yet (set_token_table / a penalty first)" );
            m->tokenTable()->read( row, out );
        }, static_cast<Runner*>( h )->model );
    } );
}
/// The bias table of the step-level calls that follow (Gemma.h: setTokenBias): every value `fill`, then values[j] at ids[j]; n < 0 turns the bias off.  replace == 0
/// updates entries of a table that is on and leaves the rest (fill is not read).
HOST_API int mila_gemma_set_token_bias( void* h, float fill, const int32_t* ids, const float* values, int64_t n, int replace )
{
    return guarded( [&]
    {
        if ( n > 0 && ( !ids || !values ) ) throw std::invalid_argument( "set_token_bias: null ids / values" );
        std::visit( [&]( auto& m )
        {
            if ( n < 0 ) m->clearTokenBias();
            else if ( replace ) m->setTokenBias( fill, ids, values, static_cast<size_t>( n ) );
            else m->updateTokenBias( ids, values, static_cast<size_t>( n ) );
        }, static_cast<Runner*>( h )->model );
    } );
}
/// the bias table [vocab] to the host; *out_on = whether the bias is on
HOST_API int mila_gemma_read_token_bias( void* h, float* out, int32_t* out_on )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            if ( !m->tokenBias() ) throw std::logic_error( "read_token_bias: no bias table yet (set_token_bias first)" );
            if ( out ) m->tokenBias()->read( out );
            if ( out_on ) *out_on = m->tokenBiasOn() ? 1 : 0;
        }, static_cast<Runner*>( h )->model );
    } );
}
/// The token automaton of the step-level calls that follow (Gemma.h: setTokenAutomaton): class_of [vocab], next [S * C]; validated, uploaded, turned on and reset to
/// `start`.  class_of == NULL turns it off.
HOST_API int mila_gemma_set_token_automaton( void* h, const uint16_t* class_of, int64_t vocab, const uint16_t* next, int S, int C, int start )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            if ( !class_of ) { m->clearTokenAutomaton(); return; }
            if ( !next || vocab < 0 || S < 0 || C < 0 ) throw std::invalid_argument( "set_token_automaton: null table or negative size" );
            TokenAutomaton a;
            a.num_states = S; a.num_classes = C; a.start = start;
            a.class_of.assign( class_of, class_of + vocab );
            a.next.assign( next, next + static_cast<size_t>( S ) * static_cast<size_t>( C ) );
            m->setTokenAutomaton( a );
        }, static_cast<Runner*>( h )->model );
    } );
}
/// the state back to `start` and the effective table composed for it
HOST_API int mila_gemma_reset_token_automaton( void* h )
{
    return guarded( [&] { std::visit( [&]( auto& m ) { m->resetTokenAutomaton(); }, static_cast<Runner*>( h )->model ); } );
}
/// *out_state = the state word (a synchronous read), *out_on = whether an automaton is on; out_eff (may be NULL): the effective table [vocab]
HOST_API int mila_gemma_token_automaton_state( void* h, int32_t* out_state, int32_t* out_on, float* out_eff )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            if ( out_state ) *out_state = m->tokenAutomatonState();
            if ( out_on ) *out_on = m->tokenAutomatonOn() ? 1 : 0;
            if ( out_eff ) m->tokenAutomaton()->read( out_eff );
        }, static_cast<Runner*>( h )->model );
    } );
}
HOST_API int mila_gemma_set_active( void* h, int b, int active, int32_t token )
{
    return guarded( [&] { std::visit( [&]( auto& m ) { m->setRowActive( b, active != 0 ); if ( token >= 0 ) m->setRowToken( b, token ); }, static_cast<Runner*>( h )->model ); } );
}
HOST_API int mila_gemma_reset_row( void* h, int b )
{
    return guarded( [&] { std::visit( [&]( auto& m ) { m->resetRow( b ); }, static_cast<Runner*>( h )->model ); } );
}
/// GemmaTransformer::rewindKvCacheRow: *accepted = 1 and row b goes on from `position`, or 0 (out of range; on a ring model: the row's rings no longer hold what a
/// continuation from `position` reads) and nothing changed
HOST_API int mila_gemma_rewind_row( void* h, int b, int64_t position, int64_t written, int* accepted )
{
    return guarded( [&]
    {
        if ( !accepted ) throw std::invalid_argument( "mila_gemma_rewind_row: null result" );
        std::visit( [&]( auto& m ) { *accepted = m->rewindKvCacheRow( b, position, written ) ? 1 : 0; }, static_cast<Runner*>( h )->model );
    } );
}
/// GemmaTransformer::forkRow (whole != 0: caches [0, len), logits and position, directly behind row src's prefill of len tokens) or forkRowPrefix (caches only, from
/// any row at a position >= len)
HOST_API int mila_gemma_fork_row( void* h, int src, unsigned dst_mask, int64_t len, int whole )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            if ( whole ) m->forkRow( src, dst_mask, len ); else m->forkRowPrefix( src, dst_mask, len );
            m->context()->synchronize();
        }, static_cast<Runner*>( h )->model );
    } );
}
/// one step over rows 0 .. B - 1.  mode 1: eager launches, 2: graph replay (captured on first use and when B, the sampler tail or the live-length bucket change).
/// greedy != 0: the step ends with the rows sampler tail (next token + position bump of every active row); 0: it ends at the logits, positions bumped.
/// max_position: the largest position among the active rows.  Outputs (each may be NULL): logits [B, vocab], tokens [B], positions [B] AFTER the step.
/// draws != NULL (greedy == 0 only): B uniform draws, one per row -- the step ends with the radix sampler over the rows at (temperature, top_k, top_p): next token
/// and position bump of every active row (GemmaTransformer::setRowsSampling); NULL: no sampler in the step
static int decode_rows_impl( void* h, int B, int64_t max_position, int mode, int greedy, float temperature, int top_k, float top_p, const float* draws, float* host_logits,
                             int32_t* host_tokens, int32_t* host_positions )
{
    return guarded( [&]
    {
        auto* r = static_cast<Runner*>( h );
        std::visit( [&]( auto& m )
        {
            if ( mode != 1 && mode != 2 ) throw std::invalid_argument( "decode_rows: mode must be 1 (eager) or 2 (graph)" );
            if ( draws && !greedy )
            {
                typename std::remove_reference_t<decltype( *m )>::SamplingParams sp; sp.temperature = temperature; sp.top_k = top_k; sp.top_p = top_p;
                r->applyFilters( sp );
                m->setRowsSampling( sp, r->stepDraws( draws, B ) );
            }
            else m->setRowsSampling( std::nullopt, nullptr );
            if ( mode == 1 ) m->decodeRows( B, max_position, greedy != 0 );
            else { m->ensureGraphRows( B, max_position, greedy != 0 ); m->replayGraphRows(); }
            auto st = m->context()->getStream();
            if ( host_logits ) Compute::rocmCheck( mila_cdna4_memcpy_d2h( host_logits, m->rowsLogits().data(), static_cast<size_t>( B ) * m->config().vocab_size * 4, st ) );
            if ( host_tokens ) Compute::rocmCheck( mila_cdna4_memcpy_d2h( host_tokens, m->rowsTokens().data(), static_cast<size_t>( B ) * 4, st ) );
            if ( host_positions ) Compute::rocmCheck( mila_cdna4_memcpy_d2h( host_positions, m->rowsPositions().data(), static_cast<size_t>( B ) * 4, st ) );
            m->context()->synchronize();
        }, r->model );
    } );
}
HOST_API int mila_gemma_decode_rows( void* h, int B, int64_t max_position, int mode, int greedy, float* host_logits, int32_t* host_tokens, int32_t* host_positions )
{
    return decode_rows_impl( h, B, max_position, mode, greedy, 1.0f, 0, 1.0f, nullptr, host_logits, host_tokens, host_positions );
}
/// mila_gemma_decode_rows ending in the stochastic rows tail: draws[ b ] is row b's uniform draw
HOST_API int mila_gemma_decode_rows_sampled( void* h, int B, int64_t max_position, int mode, float temperature, int top_k, float top_p, const float* draws, float* host_logits,
                                             int32_t* host_tokens, int32_t* host_positions )
{
    if ( !draws ) { g_err = "invalid_argument: decode_rows_sampled: null draws"; return MILA_E_INVALID_ARGUMENT; }
    return decode_rows_impl( h, B, max_position, mode, 0, temperature, top_k, top_p, draws, host_logits, host_tokens, host_positions );
}
/// mila_gemma_decode_rows (draws == NULL) or mila_gemma_decode_rows_sampled (draws != NULL) with token log-probabilities in the step: out_logprob [B] and
/// out_ids / out_logprobs [B, top_n] of the tokens the tail chose.  An inactive row's entries are whatever an earlier step left there.  The setting is off again on return.
HOST_API int mila_gemma_decode_rows_logprobs( void* h, int B, int64_t max_position, int mode, int greedy, float temperature, int top_k, float top_p, const float* draws, int top_n,
                                              float* host_logits, int32_t* host_tokens, int32_t* host_positions, float* out_logprob, int32_t* out_ids, float* out_logprobs )
{
    if ( top_n < 0 ) { g_err = "invalid_argument: decode_rows_logprobs: top_n must be 0 .. 20"; return MILA_E_INVALID_ARGUMENT; }
    int rc = mila_gemma_set_step_logprobs( h, top_n );
    if ( rc ) return rc;
    rc = decode_rows_impl( h, B, max_position, mode, draws ? 0 : greedy, temperature, top_k, top_p, draws, host_logits, host_tokens, host_positions );
    if ( !rc ) rc = guarded( [&] { read_logprobs( static_cast<Runner*>( h ), B, top_n, out_logprob, out_ids, out_logprobs ); } );
    const std::string err = g_err;
    (void)mila_gemma_set_step_logprobs( h, -1 );
    g_err = err;
    return rc;
}
/// out[0] = captures of the rows graph so far, out[1] = kernel nodes of the captured rows step
HOST_API int mila_gemma_rows_graph_info( void* h, int64_t* out )
{
    return guarded( [&] { std::visit( [&]( auto& m ) { out[ 0 ] = (int64_t)m->graphRowsCaptureCount(); out[ 1 ] = (int64_t)m->graphRowsNodeCount(); }, static_cast<Runner*>( h )->model ); } );
}
/// ROW REQUESTS for the rows steps that follow (GemmaTransformer::setRowsRequests): params = n x 7 floats, row b's temperature (<= 0: greedy), top_k, top_p, min_p,
/// repetition_penalty, presence_penalty, frequency_penalty; draws = one uniform draw per row (NULL: zeros), kept in the runner's host-visible words, which
/// mila_gemma_decode_rows_sampled rewrites per call.  n == 0 clears the requests: the rows step takes the shared parameters again.
HOST_API int mila_gemma_set_rows_requests( void* h, const float* params, int n, const float* draws )
{
    return guarded( [&]
    {
        auto* r = static_cast<Runner*>( h );
        std::visit( [&]( auto& m )
        {
            if ( n == 0 ) { m->clearRowsRequests(); return; }
            if ( !params || n < 0 || n > Runner::kStepDraws ) throw std::invalid_argument( "set_rows_requests: 1 .. 4 requests of 7 values" );
            std::vector<typename std::remove_reference_t<decltype( *m )>::SamplingParams> sp( static_cast<size_t>( n ) );
            for ( int b = 0; b < n; ++b )
            {
                const float* q = params + 7 * b;
                auto& s = sp[ static_cast<size_t>( b ) ];
                s.temperature = q[ 0 ]; s.top_k = static_cast<int>( q[ 1 ] ); s.top_p = q[ 2 ];
                s.min_p = q[ 3 ]; s.repetition_penalty = q[ 4 ]; s.presence_penalty = q[ 5 ]; s.frequency_penalty = q[ 6 ];
            }
            const float zeros[ Runner::kStepDraws ] = { 0.0f, 0.0f, 0.0f, 0.0f };
            m->setRowsRequests( sp, r->stepDraws( draws ? draws : zeros, n ) );
        }, r->model );
    } );
}
/// row b's bias table for the requests samplers: every value `fill`, then values[ j ] at ids[ j ]; n < 0 clears the row's bias
HOST_API int mila_gemma_set_row_token_bias( void* h, int b, float fill, const int32_t* ids, const float* values, int64_t n )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m ) { if ( n < 0 ) m->clearRowTokenBias( b ); else m->setRowTokenBias( b, fill, ids, values, static_cast<size_t>( n ) ); }, static_cast<Runner*>( h )->model );
    } );
}
/// row b's automaton for the requests step (mila_gemma_set_token_automaton's arguments); class_of == NULL clears it.  Set it BEFORE the row's bias.
HOST_API int mila_gemma_set_row_token_automaton( void* h, int b, const uint16_t* class_of, int64_t vocab, const uint16_t* next, int S, int C, int start )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            if ( !class_of ) { m->clearRowTokenAutomaton( b ); return; }
            if ( !next || vocab < 0 || S < 0 || C < 0 ) throw std::invalid_argument( "set_row_token_automaton: null table or negative size" );
            TokenAutomaton a;
            a.num_states = S; a.num_classes = C; a.start = start;
            a.class_of.assign( class_of, class_of + vocab );
            a.next.assign( next, next + static_cast<size_t>( S ) * static_cast<size_t>( C ) );
            m->setRowTokenAutomaton( b, a );
        }, static_cast<Runner*>( h )->model );
    } );
}
/// *out_state = row b's state word (a synchronous read), *out_on = whether the row has an automaton; out_eff (may be NULL): the row's effective table [vocab]
HOST_API int mila_gemma_row_token_automaton_state( void* h, int b, int32_t* out_state, int32_t* out_on, float* out_eff )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            const auto s = m->rowTokenAutomatonState( b );
            if ( out_state ) *out_state = s.value_or( 0 );
            if ( out_on ) *out_on = s ? 1 : 0;
            if ( out_eff )
            {
                if ( !m->rowTokenBias() ) throw std::logic_error( "row_token_automaton_state: no row table was set" );
                m->rowTokenBias()->read( b, out_eff );
            }
        }, static_cast<Runner*>( h )->model );
    } );
}
/// the sampler tail of the rows step (which = 0) or of the chain step (which = 1) for the calls that follow -- the timing loops among them: draws = n uniform draws,
/// one per row, kept in the runner's host-visible words; draws == NULL clears it (mila_gemma_decode_rows / mila_gemma_chain_decode set it per call themselves)
HOST_API int mila_gemma_set_step_sampling( void* h, int which, float temperature, int top_k, float top_p, const float* draws, int n )
{
    return guarded( [&]
    {
        auto* r = static_cast<Runner*>( h );
        std::visit( [&]( auto& m )
        {
            std::optional<typename std::remove_reference_t<decltype( *m )>::SamplingParams> sp;
            const float* dev = nullptr;
            if ( draws ) { sp.emplace(); sp->temperature = temperature; sp->top_k = top_k; sp->top_p = top_p; dev = r->stepDraws( draws, n ); }
            if ( sp && which == 0 ) r->applyFilters( *sp );      // (the chain step takes none)
            if ( which == 0 ) m->setRowsSampling( sp, dev ); else m->setChainSampling( sp, dev );
        }, r->model );
    } );
}
static int time_decode_rows_impl( void* h, int B, int64_t start_position, int steps, int warmup, bool greedy, double* out );
/// `steps` greedy graph replays of a B-row step with every row active from `start_position` (the caches hold whatever they hold: a timing loop), after `warmup`:
/// out[0] = wall ms per step, out[1] = device ms per step
HOST_API int mila_gemma_time_decode_rows( void* h, int B, int64_t start_position, int steps, int warmup, double* out )
{
    return time_decode_rows_impl( h, B, start_position, steps, warmup, true, out );
}
/// the same loop over the NON-greedy step: it ends in the stochastic rows tail when mila_gemma_set_step_sampling set one, at the logits and the position bump otherwise
HOST_API int mila_gemma_time_decode_rows_stochastic( void* h, int B, int64_t start_position, int steps, int warmup, double* out )
{
    return time_decode_rows_impl( h, B, start_position, steps, warmup, false, out );
}
static int time_decode_rows_impl( void* h, int B, int64_t start_position, int steps, int warmup, bool greedy, double* out )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            auto* ctx = m->context();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx->getStream() );
            for ( int b = 0; b < B; ++b ) { m->setRowPosition( b, start_position ); m->setRowToken( b, 17 + b ); m->setRowActive( b, true ); }
            int64_t pos = start_position;
            auto step = [&] { m->ensureGraphRows( B, pos, greedy ); m->replayGraphRows(); ++pos; };
            for ( int i = 0; i < warmup; ++i ) step();
            ctx->synchronize();
            hipEvent_t e0, e1;
            hipCheck( hipEventCreate( &e0 ), "hipEventCreate" );
            hipCheck( hipEventCreate( &e1 ), "hipEventCreate" );
            const auto t0 = std::chrono::steady_clock::now();
            hipCheck( hipEventRecord( e0, s ), "hipEventRecord" );
            for ( int i = 0; i < steps; ++i ) step();
            hipCheck( hipEventRecord( e1, s ), "hipEventRecord" );
            ctx->synchronize();
            const auto t1 = std::chrono::steady_clock::now();
            float ms = 0;
            hipCheck( hipEventElapsedTime( &ms, e0, e1 ), "hipEventElapsedTime" );
            (void)hipEventDestroy( e0 ); (void)hipEventDestroy( e1 );
            out[ 0 ] = std::chrono::duration<double, std::milli>( t1 - t0 ).count() / steps;
            out[ 1 ] = static_cast<double>( ms ) / steps;
        }, static_cast<Runner*>( h )->model );
    } );
}

// ---- chain decode: consecutive positions of ONE sequence (GemmaConfig::draft_tokens > 0) ----------------------------------------------------------------
/// one chain step: tokens[ 0 ] = the token at `position`, tokens[ 1 .. T - 1 ] = the drafts behind it.  mode 1: eager launches, 2: graph replay (captured on first use
/// and when T or the live-length bucket change; the device position word is set to `position` either way).  Outputs (each may be NULL): logits [T, vocab];
/// out[ 0 ] = count, out[ 1 .. count ] = the accepted tokens, out[ T + 1 ] = the position word after the step (out holds T + 2 words)
/// draws != NULL: T uniform draws -- the step verifies the drafts against samples (GemmaTransformer::setChainSampling); NULL: the greedy chain step
static int chain_decode_impl( void* h, const int32_t* tokens, int T, int64_t position, int mode, float temperature, int top_k, float top_p, const float* draws, float* host_logits,
                              int32_t* out )
{
    return guarded( [&]
    {
        auto* r = static_cast<Runner*>( h );
        std::visit( [&]( auto& m )
        {
            if ( mode != 1 && mode != 2 ) throw std::invalid_argument( "chain_decode: mode must be 1 (eager) or 2 (graph)" );
            if ( !tokens ) throw std::invalid_argument( "chain_decode: null tokens" );
            if ( draws )
            {
                typename std::remove_reference_t<decltype( *m )>::SamplingParams sp; sp.temperature = temperature; sp.top_k = top_k; sp.top_p = top_p;
                m->setChainSampling( sp, r->stepDraws( draws, T ) );
            }
            else m->setChainSampling( std::nullopt, nullptr );
            m->setChainDrafts( tokens, T );
            if ( mode == 1 ) m->decodeChain( T, position );
            else { m->ensureGraphChain( T, position ); m->setDevicePosition( position ); m->replayGraphChain(); }
            auto st = m->context()->getStream();
            if ( host_logits ) Compute::rocmCheck( mila_cdna4_memcpy_d2h( host_logits, m->chainLogits().data(), static_cast<size_t>( T ) * m->config().vocab_size * 4, st ) );
            if ( out )
            {
                for ( int i = 0; i < T + 2; ++i ) out[ i ] = 0;
                Compute::rocmCheck( mila_cdna4_memcpy_d2h( out, m->chainResult().data(), static_cast<size_t>( T + 1 ) * 4, st ) );
                m->context()->synchronize();
                out[ T + 1 ] = static_cast<int32_t>( m->devicePosition() );
                for ( int i = out[ 0 ] + 1; i <= T; ++i ) out[ i ] = 0;      // words past the accepted run are left over from earlier steps
            }
            m->context()->synchronize();
        }, r->model );
    } );
}
HOST_API int mila_gemma_chain_decode( void* h, const int32_t* tokens, int T, int64_t position, int mode, float* host_logits, int32_t* out )
{
    return chain_decode_impl( h, tokens, T, position, mode, 1.0f, 0, 1.0f, nullptr, host_logits, out );
}
/// mila_gemma_chain_decode verifying against samples: draws[ t ] is row t's uniform draw
HOST_API int mila_gemma_chain_decode_sampled( void* h, const int32_t* tokens, int T, int64_t position, int mode, float temperature, int top_k, float top_p, const float* draws,
                                              float* host_logits, int32_t* out )
{
    if ( !draws ) { g_err = "invalid_argument: chain_decode_sampled: null draws"; return MILA_E_INVALID_ARGUMENT; }
    return chain_decode_impl( h, tokens, T, position, mode, temperature, top_k, top_p, draws, host_logits, out );
}
/// mila_gemma_chain_decode (draws == NULL) or mila_gemma_chain_decode_sampled with token log-probabilities in the step: out_logprob [T] and out_ids / out_logprobs
/// [T, top_n]; rows 0 .. count - 1 (the accepted tokens, count = out[ 0 ]) are this step's, the others are whatever an earlier step left there.  Off again on return.
HOST_API int mila_gemma_chain_decode_logprobs( void* h, const int32_t* tokens, int T, int64_t position, int mode, float temperature, int top_k, float top_p, const float* draws,
                                               int top_n, float* host_logits, int32_t* out, float* out_logprob, int32_t* out_ids, float* out_logprobs )
{
    if ( top_n < 0 ) { g_err = "invalid_argument: chain_decode_logprobs: top_n must be 0 .. 20"; return MILA_E_INVALID_ARGUMENT; }
    int rc = mila_gemma_set_step_logprobs( h, top_n );
    if ( rc ) return rc;
    rc = chain_decode_impl( h, tokens, T, position, mode, temperature, top_k, top_p, draws, host_logits, out );
    if ( !rc ) rc = guarded( [&] { read_logprobs( static_cast<Runner*>( h ), T, top_n, out_logprob, out_ids, out_logprobs ); } );
    const std::string err = g_err;
    (void)mila_gemma_set_step_logprobs( h, -1 );
    g_err = err;
    return rc;
}
/// out[0] = captures of the chain graph so far, out[1] = kernel nodes of the captured chain step, out[2] = its rows
HOST_API int mila_gemma_chain_graph_info( void* h, int64_t* out )
{
    return guarded( [&] { std::visit( [&]( auto& m ) { out[ 0 ] = (int64_t)m->graphChainCaptureCount(); out[ 1 ] = (int64_t)m->graphChainNodeCount(); out[ 2 ] = m->graphChainRows(); },
                                      static_cast<Runner*>( h )->model ); } );
}
/// `steps` graph replays of a T-row chain step from `start_position` after `warmup` (a timing loop: the caches hold whatever they hold, the drafts are whatever the
/// token words hold, and every step advances by what it accepts -- at most T, so start_position + (steps + warmup) * T must fit the sequence length; the step's tail is
/// the greedy one unless mila_gemma_set_step_sampling set the sampling one):
/// out[0] = wall ms per step, out[1] = device ms per step
HOST_API int mila_gemma_time_chain_decode( void* h, int T, int64_t start_position, int steps, int warmup, double* out )
{
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            auto* ctx = m->context();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx->getStream() );
            const int64_t last = start_position + static_cast<int64_t>( steps + warmup ) * T;
            // the replays are not checked one by one (what a step accepts is known on the device only): the whole run must fit, every step taken as T positions
            if ( steps < 1 || warmup < 0 || start_position < 0 || last > m->maxSeq() ) throw std::invalid_argument( "time_chain_decode: the run would pass the built sequence length" );
            if ( m->bandBucket( start_position ) != m->bandBucket( last - 1 ) ) throw std::invalid_argument( "time_chain_decode: the run would leave its live-length bucket" );
            const int32_t toks[ 4 ] = { 17, 18, 19, 20 };
            m->setChainDrafts( toks, T );
            m->captureGraphChain( T, start_position );
            for ( int i = 0; i < warmup; ++i ) m->replayGraphChain();
            ctx->synchronize();
            hipEvent_t e0, e1;
            hipCheck( hipEventCreate( &e0 ), "hipEventCreate" );
            hipCheck( hipEventCreate( &e1 ), "hipEventCreate" );
            const auto t0 = std::chrono::steady_clock::now();
            hipCheck( hipEventRecord( e0, s ), "hipEventRecord" );
            for ( int i = 0; i < steps; ++i ) m->replayGraphChain();
            hipCheck( hipEventRecord( e1, s ), "hipEventRecord" );
            ctx->synchronize();
            const auto t1 = std::chrono::steady_clock::now();
            float ms = 0;
            hipCheck( hipEventElapsedTime( &ms, e0, e1 ), "hipEventElapsedTime" );
            (void)hipEventDestroy( e0 ); (void)hipEventDestroy( e1 );
            out[ 0 ] = std::chrono::duration<double, std::milli>( t1 - t0 ).count() / steps;
            out[ 1 ] = static_cast<double>( ms ) / steps;
        }, static_cast<Runner*>( h )->model );
    } );
}

/// out[0] = wall ms per step (host clock around the timed region, stream synchronised both sides)
/// out[1] = device ms per step (HIP events on the model stream)
HOST_API int mila_gemma_time_decode( void* h, int64_t start_position, int steps, int warmup, int mode, double* out )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        int32_t tok = 17;
        upload_tokens( r, &tok, 1 );
        std::visit( [&]( auto& m )
        {
            auto* ctx = m->context();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx->getStream() );
            // every step ends with the greedy device sampler writing the next token: a real autoregressive loop
            m->setSampleInGraph( true );
            if ( mode == 2 ) m->ensureGraph( *r->tokens, start_position );
            if ( mode == 2 ) m->setDevicePosition( start_position );
            auto step = [&]( int64_t pos )
            {
                if ( mode == 0 ) { m->decode( *r->tokens, pos ); m->sampleGreedy( *r->tokens ); }
                else if ( mode == 1 ) { m->decodeFused( *r->tokens, pos ); m->sampleGreedy( *r->tokens ); }
                else { m->ensureGraph( *r->tokens, pos ); m->replayGraph(); }
                if ( mode != 2 && m->stepLogprobs() ) m->enqueueStepLogprobs( r->tokens->data() );      // (the captured step runs them itself)
            };
            int64_t pos = start_position;
            for ( int i = 0; i < warmup; ++i ) step( pos++ );
            ctx->synchronize();
            hipEvent_t e0, e1;
            hipCheck( hipEventCreate( &e0 ), "hipEventCreate" );
            hipCheck( hipEventCreate( &e1 ), "hipEventCreate" );
            const auto t0 = std::chrono::steady_clock::now();
            hipCheck( hipEventRecord( e0, s ), "hipEventRecord" );
            for ( int i = 0; i < steps; ++i ) step( pos++ );
            hipCheck( hipEventRecord( e1, s ), "hipEventRecord" );
            ctx->synchronize();
            const auto t1 = std::chrono::steady_clock::now();
            float ms = 0;
            hipCheck( hipEventElapsedTime( &ms, e0, e1 ), "hipEventElapsedTime" );
            (void)hipEventDestroy( e0 ); (void)hipEventDestroy( e1 );
            out[ 0 ] = std::chrono::duration<double, std::milli>( t1 - t0 ).count() / steps;
            out[ 1 ] = static_cast<double>( ms ) / steps;
        }, r->model );
    } );
}

/// Average launch duration of the dominant kernel (fc_gate_up fused matvec) measured with HIP events on
/// the model stream: `rounds` passes over all layers' weights (so no pass re-reads a cached matrix).
/// out[0] = average microseconds per launch, out[1] = algorithmic bytes per launch
HOST_API int mila_gemma_time_dominant_kernel( void* h, int rounds, double* out )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            auto* ctx = m->context();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx->getStream() );
            const size_t L = m->layers().size();
            for ( size_t i = 0; i < L; ++i ) m->launchDominant( i );
            ctx->synchronize();
            hipEvent_t e0, e1;
            hipCheck( hipEventCreate( &e0 ), "hipEventCreate" );
            hipCheck( hipEventCreate( &e1 ), "hipEventCreate" );
            hipCheck( hipEventRecord( e0, s ), "hipEventRecord" );
            for ( int k = 0; k < rounds; ++k )
                for ( size_t i = 0; i < L; ++i ) m->launchDominant( i );
            hipCheck( hipEventRecord( e1, s ), "hipEventRecord" );
            ctx->synchronize();
            float ms = 0;
            hipCheck( hipEventElapsedTime( &ms, e0, e1 ), "hipEventElapsedTime" );
            (void)hipEventDestroy( e0 ); (void)hipEventDestroy( e1 );
            out[ 0 ] = static_cast<double>( ms ) * 1e3 / ( static_cast<double>( rounds ) * L );
            double bytes = 0;
            for ( size_t i = 0; i < L; ++i ) bytes += m->dominantBytes( i );
            out[ 1 ] = bytes / static_cast<double>( L );
        }, r->model );
    } );
}

/// a long prompt as the L6 caller feeds it (Gemma.ixx:234-267 prefill in chunks of the built prefill size, positions p0 .. p0 + n): device time of the whole
/// chunked prefill of total_T tokens from an empty cache, in ms.  The caches hold total_T positions afterwards (decode can continue at total_T).
HOST_API int mila_gemma_time_prefill_chunked( void* h, int64_t total_T, double* out_ms )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        if ( total_T <= 0 ) throw std::invalid_argument( "time_prefill_chunked: empty prompt" );
        std::vector<int32_t> toks( static_cast<size_t>( total_T ) );
        for ( int64_t i = 0; i < total_T; ++i ) toks[ i ] = static_cast<int32_t>( ( i * 7919 + 13 ) % 1000 );
        std::visit( [&]( auto& m )
        {
            auto* ctx = m->context();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx->getStream() );
            Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource> dev( ctx->getDeviceId(), shape_t{ 1, total_T } );
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( dev.rawData(), toks.data(), static_cast<size_t>( total_T ) * 4, ctx->getStream() ) );
            m->resetKVCache();
            ctx->synchronize();
            hipEvent_t e0, e1;
            hipCheck( hipEventCreate( &e0 ), "hipEventCreate" );
            hipCheck( hipEventCreate( &e1 ), "hipEventCreate" );
            hipCheck( hipEventRecord( e0, s ), "hipEventRecord" );
            m->prefillFrom( dev, total_T, 0 );
            hipCheck( hipEventRecord( e1, s ), "hipEventRecord" );
            ctx->synchronize();
            float ms = 0;
            hipCheck( hipEventElapsedTime( &ms, e0, e1 ), "hipEventElapsedTime" );
            (void)hipEventDestroy( e0 ); (void)hipEventDestroy( e1 );
            *out_ms = static_cast<double>( ms );
        }, r->model );
    } );
}

HOST_API int mila_gemma_time_prefill( void* h, int64_t T, int reps, double* out_ms )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        std::vector<int32_t> toks( static_cast<size_t>( T ) );
        for ( int64_t i = 0; i < T; ++i ) toks[ i ] = static_cast<int32_t>( ( i * 7919 + 13 ) % 1000 );
        upload_tokens( r, toks.data(), T );
        std::visit( [&]( auto& m )
        {
            auto* ctx = m->context();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx->getStream() );
            m->prefill( *r->tokens, T, 0 );
            ctx->synchronize();
            hipEvent_t e0, e1;
            hipCheck( hipEventCreate( &e0 ), "hipEventCreate" );
            hipCheck( hipEventCreate( &e1 ), "hipEventCreate" );
            hipCheck( hipEventRecord( e0, s ), "hipEventRecord" );
            for ( int i = 0; i < reps; ++i ) m->prefill( *r->tokens, T, 0 );
            hipCheck( hipEventRecord( e1, s ), "hipEventRecord" );
            ctx->synchronize();
            float ms = 0;
            hipCheck( hipEventElapsedTime( &ms, e0, e1 ), "hipEventElapsedTime" );
            (void)hipEventDestroy( e0 ); (void)hipEventDestroy( e1 );
            *out_ms = static_cast<double>( ms ) / reps;
        }, r->model );
    } );
}

/// mila_gemma_time_prefill for prefillScored: rows [first_row, T) are scored (argmax on), each row's target the chunk's next token
HOST_API int mila_gemma_time_score_from( void* h, int64_t T, int64_t first_row, int reps, double* out_ms )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        if ( T <= 0 || T > r->max_prefill ) throw std::invalid_argument( "time_score: chunk length out of range" );
        if ( reps < 1 ) throw std::invalid_argument( "time_score: reps must be positive" );
        std::vector<int32_t> toks( static_cast<size_t>( T ) ), tg( static_cast<size_t>( T ) );
        for ( int64_t i = 0; i < T; ++i ) toks[ i ] = static_cast<int32_t>( ( i * 7919 + 13 ) % 1000 );
        for ( int64_t i = 0; i < T; ++i ) tg[ i ] = i + 1 < T ? toks[ i + 1 ] : -1;
        upload_tokens( r, toks.data(), T );
        std::visit( [&]( auto& m )
        {
            auto* ctx = m->context();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx->getStream() );
            Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource> targets( ctx->getDeviceId(), shape_t{ T } );
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( targets.rawData(), tg.data(), static_cast<size_t>( T ) * 4, ctx->getStream() ) );
            m->prefillScored( *r->tokens, T, 0, targets.data(), first_row, true );
            ctx->synchronize();
            hipEvent_t e0, e1;
            hipCheck( hipEventCreate( &e0 ), "hipEventCreate" );
            hipCheck( hipEventCreate( &e1 ), "hipEventCreate" );
            hipCheck( hipEventRecord( e0, s ), "hipEventRecord" );
            for ( int i = 0; i < reps; ++i ) m->prefillScored( *r->tokens, T, 0, targets.data(), first_row, true );
            hipCheck( hipEventRecord( e1, s ), "hipEventRecord" );
            ctx->synchronize();
            float ms = 0;
            hipCheck( hipEventElapsedTime( &ms, e0, e1 ), "hipEventElapsedTime" );
            (void)hipEventDestroy( e0 ); (void)hipEventDestroy( e1 );
            *out_ms = static_cast<double>( ms ) / reps;
        }, r->model );
    } );
}
/// every row of the chunk scored
HOST_API int mila_gemma_time_score( void* h, int64_t T, int reps, double* out_ms ) { return mila_gemma_time_score_from( h, T, 0, reps, out_ms ); }

/// greedy generation: feeds `first_token` at `start_position`, then n_tokens - 1 more steps, each consuming the
/// token the device sampler produced; returns the sampled ids (host) -- mode as in mila_gemma_decode
HOST_API int mila_gemma_generate( void* h, int32_t first_token, int64_t start_position, int n_tokens, int mode, int32_t* host_out )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        upload_tokens( r, &first_token, 1 );
        std::visit( [&]( auto& m )
        {
            auto* ctx = m->context();
            m->setSampleInGraph( true );
            if ( mode == 2 ) m->ensureGraph( *r->tokens, start_position );
            if ( mode == 2 ) m->setDevicePosition( start_position );
            for ( int i = 0; i < n_tokens; ++i )
            {
                const int64_t pos = start_position + i;
                if ( mode == 0 ) { m->decode( *r->tokens, pos ); m->sampleGreedy( *r->tokens ); }
                else if ( mode == 1 ) { m->decodeFused( *r->tokens, pos ); m->sampleGreedy( *r->tokens ); }
                else { m->ensureGraph( *r->tokens, pos ); m->replayGraph(); }
                Compute::rocmCheck( mila_cdna4_memcpy_d2h( host_out + i, r->tokens->data(), 4, ctx->getStream() ) );
                ctx->synchronize();
            }
        }, r->model );
    } );
}

/// Stochastic generation: like mila_gemma_generate with the multinomial device sampler; the per-step uniform comes from a host mt19937( seed ) as in the
/// reference's generate loop.  pipeline 0: sample_stochastic_* (the 16-ary search), eager, modes 0 and 1; pipeline 1: the radix pipeline -- eager behind the step in
/// modes 0 and 1, as the tail of the captured step in mode 2 (the draw travels through a host-visible ring, the token comes back through another).
/// temperature <= 0 degenerates to greedy in modes 0 and 1.
HOST_API int mila_gemma_generate_sampled( void* h, int32_t first_token, int64_t start_position, int n_tokens, int mode, int pipeline, float temperature, int top_k,
                                          float top_p, uint32_t seed, int32_t* host_out )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        if ( pipeline != 0 && pipeline != 1 ) throw std::invalid_argument( "generate_sampled: pipeline must be 0 (16-ary search) or 1 (radix)" );
        if ( mode != 0 && mode != 1 && !( mode == 2 && pipeline == 1 ) )
            throw std::invalid_argument( "generate_sampled: mode must be 0 (reference order) or 1 (fused), or 2 (graph) with the radix pipeline" );
        upload_tokens( r, &first_token, 1 );
        std::mt19937 rng( seed );
        std::uniform_real_distribution<float> uni( 0.0f, 1.0f );
        std::visit( [&]( auto& m )
        {
            auto* ctx = m->context();
            typename std::remove_reference_t<decltype( *m )>::SamplingParams sp;
            sp.temperature = temperature; sp.top_k = top_k; sp.top_p = top_p;
            r->applyFilters( sp );
            if ( sp.filtered() && pipeline != 1 ) throw std::invalid_argument( "generate_sampled: the sampling filters need the radix pipeline" );
            if ( mode != 2 )
            {
                for ( int i = 0; i < n_tokens; ++i )
                {
                    const int64_t pos = start_position + i;
                    if ( mode == 0 ) m->decode( *r->tokens, pos ); else m->decodeFused( *r->tokens, pos );
                    if ( pipeline == 1 ) m->sampleStochasticRadix( *r->tokens, sp, uni( rng ) ); else m->sampleStochastic( *r->tokens, sp, uni( rng ) );
                    Compute::rocmCheck( mila_cdna4_memcpy_d2h( host_out + i, r->tokens->data(), 4, ctx->getStream() ) );
                    ctx->synchronize();
                }
                return;
            }
            if ( !r->seq_dev )
            {
                hipCheck( hipHostMalloc( reinterpret_cast<void**>( &r->draws_host ), Runner::kRing * sizeof( float ), hipHostMallocMapped | hipHostMallocCoherent ), "hipHostMalloc (draw ring)" );
                hipCheck( hipHostMalloc( reinterpret_cast<void**>( &r->ring_host ), Runner::kRing * sizeof( unsigned long long ), hipHostMallocMapped | hipHostMallocCoherent ), "hipHostMalloc (token ring)" );
                std::memset( r->draws_host, 0, Runner::kRing * sizeof( float ) );
                std::memset( r->ring_host, 0, Runner::kRing * sizeof( unsigned long long ) );
                void* d = nullptr;
                hipCheck( hipHostGetDevicePointer( &d, r->draws_host, 0 ), "hipHostGetDevicePointer" );
                r->draws_dev = static_cast<const float*>( d );
                hipCheck( hipHostGetDevicePointer( &d, r->ring_host, 0 ), "hipHostGetDevicePointer" );
                r->ring_dev = static_cast<unsigned long long*>( d );
                r->seq_dev = std::make_unique<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>>( ctx->getDeviceId(), shape_t{ 2 } );
                Compute::rocmCheck( mila_cdna4_memset_zero( r->seq_dev->rawData(), 8, ctx->getStream() ) );
                ctx->synchronize();
            }
            // the settings are this call's: whatever happens, a later greedy or sampler-less capture must not inherit them (the capture itself stays valid)
            struct Reset { decltype( m )& net; ~Reset() { net->setGraphSampling( std::nullopt ); net->setDrawRing( nullptr, 0 ); net->setTokenRing( nullptr, 0, nullptr ); } } reset{ m };
            m->setSampleInGraph( false );
            m->setTokenRing( r->ring_dev, Runner::kRing, reinterpret_cast<unsigned long long*>( r->seq_dev->rawData() ) );
            m->setDrawRing( r->draws_dev, Runner::kRing );
            m->setGraphSampling( sp );
            m->ensureGraph( *r->tokens, start_position );
            m->setDevicePosition( start_position );
            // the device counter is the truth: an earlier call that threw between a replay and its bookkeeping must not leave this one reading the wrong slots
            Compute::rocmCheck( mila_cdna4_memcpy_d2h( &r->samples, r->seq_dev->rawData(), 8, ctx->getStream() ) );
            ctx->synchronize();
            for ( int i = 0; i < n_tokens; ++i )
            {
                m->ensureGraph( *r->tokens, start_position + i );
                const uint64_t seq = r->samples + 1;
                const float u = uni( rng );
                uint32_t bits;
                std::memcpy( &bits, &u, 4 );
                __atomic_store_n( reinterpret_cast<uint32_t*>( r->draws_host ) + ( seq % Runner::kRing ), bits, __ATOMIC_RELEASE );
                m->replayGraph();
                r->samples = seq;
                ctx->synchronize();
                const unsigned long long v = __atomic_load_n( r->ring_host + ( seq % Runner::kRing ), __ATOMIC_ACQUIRE );
                if ( ( v >> 32 ) != ( seq & 0xffffffffull ) ) throw std::runtime_error( "generate_sampled: the captured step did not publish its token" );
                host_out[ i ] = static_cast<int32_t>( static_cast<uint32_t>( v ) );
            }
        }, r->model );
    } );
}

/// model facts for the bench line: out[0] algorithmic bytes per decode token at `context`,
/// out[1] weight bytes, out[2] Linear parameter count (body), out[3] table parameter count
HOST_API int mila_gemma_info( void* h, int64_t context, double* out )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            out[ 0 ] = m->decodeBytesPerToken( context );
            out[ 1 ] = m->weightBytes();
            double p = 0;
            const auto& c = m->config();
            for ( dim_t i = 0; i < c.num_layers; ++i ) p += static_cast<double>( c.linearParamsPerLayer( c.isGlobalLayer( i ) ) );
            out[ 2 ] = p;
            out[ 3 ] = static_cast<double>( c.vocab_size ) * c.embedding_dim;
        }, r->model );
    } );
}

/// out[0..2] = getRequiredMemory(): device parameter / device state / host state bytes; out[3..5] = getMemoryStats() likewise; out[6] = the context's scratch high-water mark
HOST_API int mila_gemma_memory_stats( void* h, double* out )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            const Mila::Dnn::MemoryStats req = m->getRequiredMemory(), act = m->getMemoryStats();
            out[ 0 ] = static_cast<double>( req.device_parameter_bytes ); out[ 1 ] = static_cast<double>( req.device_state_bytes ); out[ 2 ] = static_cast<double>( req.host_state_bytes );
            out[ 3 ] = static_cast<double>( act.device_parameter_bytes ); out[ 4 ] = static_cast<double>( act.device_state_bytes ); out[ 5 ] = static_cast<double>( act.host_state_bytes );
            out[ 6 ] = static_cast<double>( m->context()->getScratchHighWaterBytes() );
        }, r->model );
    } );
}

/// nodes of the captured decode graph (0 before the first graph-mode step)
HOST_API int mila_gemma_graph_node_count( void* h, int64_t* out )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { std::visit( [&]( auto& m ) { *out = static_cast<int64_t>( m->graphNodeCount() ); }, r->model ); } );
}

/// how often the decode graph has been captured (first use + every re-capture ensureGraph() decided on, e.g. a position in another band bucket)
HOST_API int mila_gemma_graph_capture_count( void* h, int64_t* out )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { std::visit( [&]( auto& m ) { *out = static_cast<int64_t>( m->graphCaptureCount() ); }, r->model ); } );
}

/// bytes of op-owned resident prefill staging held by the layer Linears at this moment
HOST_API int mila_gemma_resident_staging_bytes( void* h, double* out )
{
    auto* r = static_cast<Runner*>( h );
    return guarded( [&] { std::visit( [&]( auto& m ) { *out = m->residentStagingBytes(); }, r->model ); } );
}

/// component names of the model, '\n'-separated, in construction order (children of each block, then temb / rmsn_final / lm_head);
/// returns the length needed (including the terminator); writes at most `cap` bytes
HOST_API int64_t mila_gemma_component_names( void* h, char* buf, int64_t cap )
{
    std::string out;
    int rc = guarded( [&]
    {
        std::visit( [&]( auto& m )
        {
            for ( auto& L : m->layers() )
            {
                out += L.getName() + "\n";
                for ( const std::string& n : L.childNames() ) out += n + "\n";
            }
            out += m->tokenEmbedding().getName() + "\n" + m->finalNorm().getName() + "\n" + m->lmHead().getName() + "\n";
        }, static_cast<Runner*>( h )->model );
    } );
    if ( rc ) return -1;
    if ( buf && cap > 0 ) { const size_t n = std::min<size_t>( out.size(), static_cast<size_t>( cap - 1 ) ); std::memcpy( buf, out.data(), n ); buf[ n ] = 0; }
    return static_cast<int64_t>( out.size() + 1 );
}

/// The leaf components used on their own, as code written against the reference uses them (construct with a name and a config,
/// setExecutionContext, build, forward): each result is compared on the host with the C-ABI launcher it resolves to, and the lifecycle
/// errors are the reference's (forward before build -> runtime_error naming the component; bad shapes -> invalid_argument).
/// Returns 0, or an error whose text says which scenario failed.
HOST_API int mila_component_scenarios( int device )
{
    return guarded( [&]
    {
        using Dev = Compute::RocmDeviceMemoryResource;
        using T16 = Tensor<TensorDataType::BF16, Dev>;
        using TI = Tensor<TensorDataType::INT32, Dev>;
        constexpr auto kD = DeviceType::Rocm;
        constexpr auto kP = TensorDataType::BF16;
        auto owned = Compute::createExecutionContext( Compute::Device::Rocm( device ) );
        auto* ctx = Compute::cast_context<kD>( owned.get() );
        const auto dev = ctx->getDeviceId();
        auto fail = [&]( const std::string& what ) { throw std::runtime_error( "component scenario failed: " + what ); };
        auto fillu = [&]( T16& t, uint64_t seed, float amp, float off ) { Compute::rocmCheck( mila_cdna4_fill_uniform_bf16( t.data(), (int64_t)t.size(), seed, amp, off, ctx->getStream() ) ); };
        auto host = [&]( const T16& t, size_t n )
        {
            std::vector<uint16_t> v( n );
            Compute::rocmCheck( mila_cdna4_memcpy_d2h( v.data(), t.rawData(), n * 2, ctx->getStream() ) );
            ctx->synchronize();
            return v;
        };
        auto expect_throw = [&]( auto&& f, bool invalid_arg, const std::string& what )
        {
            try { f(); }
            catch ( const std::invalid_argument& ) { if ( !invalid_arg ) fail( what + " (threw invalid_argument, expected runtime_error)" ); return; }
            catch ( const std::runtime_error& ) { if ( invalid_arg ) fail( what + " (threw runtime_error, expected invalid_argument)" ); return; }
            fail( what + " (did not throw)" );
        };
        const dim_t B = 2, T = 5, NH = 4, NKV = 2, HD = 64, C = NH * HD;

        // ---- Residual: forward(a, b) = a + b, component-owned output ----
        {
            Residual<kD, kP> res( "res_1", ResidualConfig{} );
            T16 a( dev, shape_t{ B, T, C } ), b( dev, shape_t{ B, T, C } ), ref( dev, shape_t{ B, T, C } );
            fillu( a, 1, 1.0f, 0.0f ); fillu( b, 2, 1.0f, 0.0f );
            res.setExecutionContext( ctx );
            expect_throw( [&] { res.forward( a, b ); }, false, "Residual::forward before build" );
            res.build( BuildContext( shape_t{ B, T, C }, RuntimeMode::Inference ) );
            auto& y = res.forward( a, b );
            Compute::rocmCheck( mila_cdna4_residual_bf16( ref.data(), a.data(), b.data(), (int64_t)a.size(), ctx->getStream() ) );
            if ( y.shape() != a.shape() || host( y, a.size() ) != host( ref, a.size() ) ) fail( "Residual::forward" );
            expect_throw( [&] { ResidualConfig().withScalingFactor( 0.0f ).validate(); }, true, "ResidualConfig scaling_factor 0" );
        }
        // ---- Swiglu<Gelu>: [.., 2H] -> [.., H] ----
        {
            Swiglu<kD, kP, ActivationType::Gelu> g( "geglu", SwigluConfig() );
            T16 x( dev, shape_t{ B, T, 2 * C } ), ref( dev, shape_t{ B, T, C } );
            fillu( x, 3, 2.0f, 0.0f );
            g.setExecutionContext( ctx );
            g.build( BuildContext( shape_t{ B, T, 2 * C }, RuntimeMode::Inference ) );
            auto& y = g.forward( x );
            Compute::rocmCheck( mila_cdna4_geglu_bf16( ref.data(), x.data(), (int)( B * T ), (int)C, ctx->getStream() ) );
            if ( y.shape() != shape_t{ B, T, C } || host( y, ref.size() ) != host( ref, ref.size() ) ) fail( "Swiglu<Gelu>::forward" );
            T16 odd( dev, shape_t{ B, T, 7 } );
            expect_throw( [&] { g.forward( odd ); }, true, "Swiglu odd width" );
        }
        // ---- Rope: prefill == decode position by position; bounds ----
        {
            const dim_t MAXS = 64;
            Rope<kD, kP> rope( "rope", RopeConfig( C, NH, NKV, MAXS ).withBase( 10000.0f ) );
            rope.setExecutionContext( ctx );
            rope.build( BuildContext( shape_t{ 1, T, C }, RuntimeMode::Inference ) );
            T16 q( dev, shape_t{ 1, T, C } ), k( dev, shape_t{ 1, T, NKV * HD } ), q1( dev, shape_t{ 1, T, C } ), k1( dev, shape_t{ 1, T, NKV * HD } );
            fillu( q, 4, 1.0f, 0.0f ); fillu( k, 5, 1.0f, 0.0f );
            Compute::rocmCheck( mila_cdna4_memcpy_d2d( q1.rawData(), q.rawData(), q.sizeInBytes(), ctx->getStream() ) );
            Compute::rocmCheck( mila_cdna4_memcpy_d2d( k1.rawData(), k.rawData(), k.sizeInBytes(), ctx->getStream() ) );
            rope.prefill( q, k, 7 );
            for ( dim_t t = 0; t < T; ++t )
            {
                auto qt = q1.slice( static_cast<size_t>( t * C ), shape_t{ 1, 1, C } );
                auto kt = k1.slice( static_cast<size_t>( t * NKV * HD ), shape_t{ 1, 1, NKV * HD } );
                rope.decode( qt, kt, 7 + t );
            }
            if ( host( q, q.size() ) != host( q1, q.size() ) || host( k, k.size() ) != host( k1, k.size() ) ) fail( "Rope::prefill vs decode" );
            expect_throw( [&] { rope.prefill( q, k, MAXS - 2 ); }, true, "Rope positions beyond the cache" );
            expect_throw( [&] { RopeConfig( C, NH, 3, MAXS ).validate(); }, true, "RopeConfig n_heads % n_kv_heads" );
        }
        // ---- GroupedQueryAttention: chunked prefill then decode == one prefill over the same tokens (same cache, same kernels' contract) ----
        {
            const dim_t MAXS = 32;
            auto mk = [&]( const char* name )
            {
                auto a = std::make_unique<GroupedQueryAttention<kD, kP>>( name, GqaConfig( C, NH, NKV ).withAttentionScale( 1.0f ) );
                a->setExecutionContext( ctx );
                a->build( BuildContext( shape_t{ 1, MAXS, ( NH + 2 * NKV ) * HD }, RuntimeMode::Inference, false, T + 1 ) );
                return a;
            };
            auto a1 = mk( "gqa" ), a2 = mk( "gqa" );
            T16 q( dev, shape_t{ 1, T + 1, C } ), k( dev, shape_t{ 1, T + 1, NKV * HD } ), v( dev, shape_t{ 1, T + 1, NKV * HD } );
            fillu( q, 6, 1.0f, 0.0f ); fillu( k, 7, 1.0f, 0.0f ); fillu( v, 8, 1.0f, 0.0f );
            auto& full = a1->prefill( q, k, v, 0 );
            auto full_h = host( full, static_cast<size_t>( ( T + 1 ) * C ) );
            a2->prefill( q.view( shape_t{ 1, T, C } ), k.view( shape_t{ 1, T, NKV * HD } ), v.view( shape_t{ 1, T, NKV * HD } ), 0 );
            auto& last = a2->decode( q.slice( static_cast<size_t>( T * C ), shape_t{ 1, 1, C } ), k.slice( static_cast<size_t>( T * NKV * HD ), shape_t{ 1, 1, NKV * HD } ),
                                     v.slice( static_cast<size_t>( T * NKV * HD ), shape_t{ 1, 1, NKV * HD } ), T );
            auto last_h = host( last, static_cast<size_t>( C ) );
            for ( dim_t i = 0; i < C; ++i )
            {
                auto f = []( uint16_t b ) { uint32_t u = (uint32_t)b << 16; float x; std::memcpy( &x, &u, 4 ); return x; };
                const float d = std::fabs( f( last_h[ i ] ) - f( full_h[ static_cast<size_t>( T * C + i ) ] ) );
                if ( !( d <= 2e-2f ) ) fail( "GroupedQueryAttention decode vs prefill row (|d| = " + std::to_string( d ) + ")" );
            }
            if ( a2->cacheLength() != T + 1 || !a2->supportsKVCache() ) fail( "GroupedQueryAttention cache bookkeeping" );
            if ( !a2->rewindKvCache( 2 ) || a2->cacheLength() != 2 || a2->rewindKvCache( 9 ) ) fail( "GroupedQueryAttention::rewindKvCache" );
            a2->resetKVCache();
            if ( a2->cacheLength() != 0 ) fail( "GroupedQueryAttention::resetKVCache" );
            expect_throw( [&] { GqaConfig( C, NH, 3 ).validate(); }, true, "GqaConfig num_heads % num_kv_heads" );
            GroupedQueryAttention<kD, kP> unbuilt( "gqa", GqaConfig( C, NH, NKV ) );
            expect_throw( [&] { unbuilt.prefill( q, k, v, 0 ); }, false, "GroupedQueryAttention::prefill before build" );
        }
        // ---- TokenEmbedding: forward(tokens) = wte[id] * scale; bf16 and FP8 tables; the tied Linear adopts the table ----
        {
            const dim_t V = 50, E = 32;
            std::vector<uint16_t> table( static_cast<size_t>( V * E ) );
            for ( size_t i = 0; i < table.size(); ++i ) { const float x = 0.01f * static_cast<float>( ( i * 37 ) % 101 ) - 0.5f; uint32_t u; std::memcpy( &u, &x, 4 ); table[ i ] = static_cast<uint16_t>( u >> 16 ); }
            std::vector<int32_t> ids{ 3, 49, 0, 17, 17, 8 };
            TI tok( dev, shape_t{ 2, 3 } );
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( tok.rawData(), ids.data(), ids.size() * 4, ctx->getStream() ) );
            TokenEmbedding<kD, TensorDataType::INT32, kP> emb( "temb", TokenEmbeddingConfig().withVocabSize( V ).withEmbeddingDim( E ).withEmbeddingScale( 2.0f ) );
            emb.setExecutionContext( ctx );
            expect_throw( [&] { emb.forward( tok ); }, false, "TokenEmbedding::forward before build" );
            emb.build( BuildContext( shape_t{ 2, 4 }, RuntimeMode::Inference ) );
            emb.loadParameter( "wte", table.data(), table.size() * 2 );
            auto& y = emb.forward( tok );
            auto yh = host( y, ids.size() * static_cast<size_t>( E ) );
            auto f = []( uint16_t b ) { uint32_t u = (uint32_t)b << 16; float x; std::memcpy( &x, &u, 4 ); return x; };
            for ( size_t t = 0; t < ids.size(); ++t )
                for ( dim_t e = 0; e < E; ++e )
                    if ( f( yh[ t * E + e ] ) != 2.0f * f( table[ static_cast<size_t>( ids[ t ] * E + e ) ] ) ) fail( "TokenEmbedding::forward (bf16 table)" );
            if ( emb.takeError() != 0 ) fail( "TokenEmbedding error flag set on valid ids" );
            TI big( dev, shape_t{ 2, 5 } );
            expect_throw( [&] { emb.forward( big ); }, false, "TokenEmbedding input beyond the built shape" );
            expect_throw( [&] { emb.loadParameter( "wte_scale", table.data(), 4 ); }, true, "wte_scale on an unquantized table" );
            // tied head: logits = x . wte^T through the SAME allocation
            Linear<kD, kP> head( "lm_head", LinearConfig( E, V ).withBias( false ) );
            head.setExecutionContext( ctx );
            head.installSharedWeight( emb.getWeightTensorShared() );
            head.build( BuildContext( shape_t{ 1, 1, E }, RuntimeMode::Inference ) );
            if ( head.getWeight().rawData() != emb.getWeightTensorShared()->rawData() || !head.hasSharedWeight() ) fail( "Linear::installSharedWeight does not alias the table" );
            // FP8 table: quantize on load, gather dequantizes with the row scale
            TokenEmbedding<kD, TensorDataType::INT32, kP, PerChannelFp8<>> q8( "temb", TokenEmbeddingConfig().withVocabSize( V ).withEmbeddingDim( E ) );
            q8.setExecutionContext( ctx );
            q8.build( BuildContext( shape_t{ 2, 4 }, RuntimeMode::Inference ) );
            q8.loadParameter( "wte", table.data(), table.size() * 2 );
            auto& y8 = q8.forward( tok );
            auto y8h = host( y8, ids.size() * static_cast<size_t>( E ) );
            for ( size_t t = 0; t < ids.size(); ++t )
                for ( dim_t e = 0; e < E; ++e )
                {
                    const float want = f( table[ static_cast<size_t>( ids[ t ] * E + e ) ] );
                    if ( std::fabs( f( y8h[ t * E + e ] ) - want ) > 0.0625f * 0.5f + 1e-3f ) fail( "TokenEmbedding::forward (FP8 table)" );   // e4m3: 3 mantissa bits, |w| <= 0.5
                }
            Linear<kD, kP, PerChannelFp8<>> head8( "lm_head", LinearConfig( E, V ).withBias( false ) );
            head8.setExecutionContext( ctx );
            head8.installSharedWeight( q8.getWeightTensorShared(), q8.getWeightScalesTensorShared() );
            head8.build( BuildContext( shape_t{ 1, 1, E }, RuntimeMode::Inference ) );
            if ( head8.getWeightScale()->rawData() != q8.getWeightScalesTensorShared()->rawData() ) fail( "Linear::installSharedWeight(weight, scales)" );
            expect_throw( [&] { head8.installSharedWeight( q8.getWeightTensorShared(), q8.getWeightScalesTensorShared() ); }, false, "installSharedWeight after build" );
        }
        // ---- GemmaBlock<kGlobal> as its own type: Tests/Dnn/Components/Transformers/Gemma/Gemma.Block.Cuda.cpp:132-262 on the same small geometry ----
        {
            using LocalBlock = GemmaBlock<kD, kP, false>;
            using GlobalBlock = GemmaBlock<kD, kP, true>;
            static_assert( LocalBlock::getDeviceType() == kD && LocalBlock::getPrecision() == kP );
            auto cfg_of = []( bool g )
            {
                GemmaBlockConfig c;
                c.model_dim = 64; c.hidden_dim = 128; c.num_heads = 4; c.num_kv_heads = g ? 1 : 2; c.head_dim = g ? 64 : 32;
                c.window = g ? 0 : 8; c.rotary_dim = g ? 32 : 0; c.rope_theta = g ? 1000000.0f : 10000.0f; c.rms_norm_eps = 1e-6f; c.max_seq = 32;
                return c;
            };
            const dim_t seq = 8;
            LocalBlock local( "gemma_local", cfg_of( false ) );
            GlobalBlock global( "gemma_global", cfg_of( true ) );
            local.setExecutionContext( ctx ); global.setExecutionContext( ctx );
            if ( local.isBuilt() || global.isBuilt() ) fail( "GemmaBlock built before build()" );                                       // ConstructLocal / ConstructGlobal
            {
                LocalBlock rank2( "gemma_local", cfg_of( false ) ); rank2.setExecutionContext( ctx );
                expect_throw( [&] { rank2.build( BuildContext( shape_t{ seq, 64 }, RuntimeMode::Inference ) ); }, true, "GemmaBlock Build_ThrowsOnNonRank3Input (:185)" );
                LocalBlock wrong( "gemma_local", cfg_of( false ) ); wrong.setExecutionContext( ctx );
                expect_throw( [&] { wrong.build( BuildContext( shape_t{ 1, seq, 65 }, RuntimeMode::Inference ) ); }, true, "GemmaBlock Build_ThrowsOnModelDimMismatch (:194)" );
            }
            // LocalGeometry_SlidingWidthsAndWindow (:206), GlobalGeometry_WidenedHeadDimAndKEqualsV (:220), HeadDim_IsDecoupledFromResidualStream (:235)
            if ( local.isGlobal() || local.headDim() != 32 || local.numKVHeads() != 2 || local.keyEqualsValue() || local.window() != 8 || local.qProjWidth() != 128 ||
                 local.kvProjWidth() != 64 || local.packedQKVWidth() != 256 ) fail( "GemmaBlock local geometry" );
            if ( !global.isGlobal() || global.headDim() != 64 || global.numKVHeads() != 1 || !global.keyEqualsValue() || global.window() != 0 || global.qProjWidth() != 256 ||
                 global.kvProjWidth() != 64 || global.packedQKVWidth() != 320 ) fail( "GemmaBlock global geometry (K = V drops the V section)" );
            if ( local.headDim() == 64 / 4 || local.qProjWidth() == 64 ) fail( "GemmaBlock head_dim must be decoupled from model_dim / num_heads" );
            // GetComponents_ReturnsCorrectChildrenSize (:249), GlobalBlock_HasSameGraphShape (:258): 7 norms + qkv_proj + rope + gqa + o_proj + res_1 + fc_gate_up + geglu + fc_down + res_2
            if ( local.childNames().size() != 16u || global.childNames().size() != 16u ) fail( "GemmaBlock children" );
            local.build( BuildContext( shape_t{ 1, seq, 64 }, RuntimeMode::Inference ) );                                                 // BuildLocal_SetsIsBuilt / AllocatesParameters
            global.build( BuildContext( shape_t{ 1, seq, 64 }, RuntimeMode::Inference ) );
            if ( !local.isBuilt() || !global.isBuilt() || local.qkv_proj->getParameterBytes() != 256u * 64u * 2u || global.qkv_proj->getParameterBytes() != 320u * 64u * 2u )
                fail( "GemmaBlock build / parameter allocation" );
            // SaveThenLoad_RestoresLayerScalar (:357): the scalar travels as a one-element F32 parameter
            const float two_and_a_half = 2.5f;
            local.loadParameter( "layer_scalar", &two_and_a_half, 4 );
            if ( local.layer_scalar != 2.5f ) fail( "GemmaBlock layer_scalar" );
            expect_throw( [&] { local.loadParameter( "layer_scalar", &two_and_a_half, 8 ); }, true, "GemmaBlock layer_scalar blob size" );
            expect_throw( [&] { local.loadParameter( "no_such", &two_and_a_half, 4 ); }, true, "GemmaBlock unknown parameter" );
            // a forward through both kinds: prefill of the chunk, then one decode step continues it (finite outputs of the right shape)
            auto fill_w = [&]( auto& blk, uint64_t seed )
            {
                for ( auto* lin : { blk.qkv_proj.get(), blk.o_proj.get(), blk.fc_gate_up.get(), blk.fc_down.get() } ) fillu( lin->getWeight(), seed++, 0.1f, 0.0f );
                for ( auto* n : { blk.input_norm.get(), blk.q_norm.get(), blk.k_norm.get(), blk.v_norm.get(), blk.post_attn_norm.get(), blk.pre_ffn_norm.get(), blk.post_ffn_norm.get() } )
                    fillu( *n->getWeight(), seed++, 0.1f, 1.0f );
            };
            // (the attention kernels serve head sizes 64 ... 512: the forward runs on the same graph with head_dim 64 / 128)
            auto fwd_cfg = [&]( bool g ) { auto c = cfg_of( g ); c.head_dim = g ? 128 : 64; return c; };
            LocalBlock flocal( "gemma_local", fwd_cfg( false ) );
            GlobalBlock fglobal( "gemma_global", fwd_cfg( true ) );
            flocal.setExecutionContext( ctx ); fglobal.setExecutionContext( ctx );
            flocal.build( BuildContext( shape_t{ 1, seq, 64 }, RuntimeMode::Inference ) );
            fglobal.build( BuildContext( shape_t{ 1, seq, 64 }, RuntimeMode::Inference ) );
            fill_w( flocal, 100 ); fill_w( fglobal, 200 );
            T16 x( dev, shape_t{ 1, seq, 64 } ), x1( dev, shape_t{ 1, 1, 64 } );
            fillu( x, 7, 1.0f, 0.0f ); fillu( x1, 8, 1.0f, 0.0f );
            for ( IDecoderLayer<kD, kP>* blk : { static_cast<IDecoderLayer<kD, kP>*>( &flocal ), static_cast<IDecoderLayer<kD, kP>*>( &fglobal ) } )
            {
                auto& y = blk->prefill( x, 0 );
                if ( y.shape() != shape_t{ 1, seq, 64 } ) fail( "GemmaBlock::prefill output shape" );
                auto yh = host( y, static_cast<size_t>( seq * 64 ) );
                auto& d = blk->decode( x1, seq );
                if ( d.shape() != shape_t{ 1, 1, 64 } ) fail( "GemmaBlock::decode output shape" );
                auto dh = host( d, 64 );
                for ( uint16_t b : yh ) if ( ( b & 0x7f80 ) == 0x7f80 ) fail( "GemmaBlock::prefill produced a non-finite value" );
                for ( uint16_t b : dh ) if ( ( b & 0x7f80 ) == 0x7f80 ) fail( "GemmaBlock::decode produced a non-finite value" );
                blk->resetKVCache();
            }
            expect_throw( [&] { flocal.decode( x, 0 ); }, true, "GemmaBlock::decode takes one token" );
        }
        ctx->synchronize();
    } );
}

// ---- L6: GemmaModel (Models/GemmaModel.ixx): fromPretrained / generate -------------------------------------------------------------
using RocmGemmaModel = GemmaModel<DeviceType::Rocm, TensorDataType::BF16>;

static GemmaModelConfig model_config_of( int policy, int64_t context, int64_t chunk, int bounded, int kv_fp8 )
{
    if ( policy < 0 || policy > 2 ) throw std::invalid_argument( "unknown weight policy" );
    GemmaModelConfig mc;
    mc.withContextLength( context ).withWeightQuantization( policy == 0 ? WeightQuantization::None : ( policy == 1 ? WeightQuantization::FP8 : WeightQuantization::FP4 ) );
    mc.withPrefillChunk( chunk ).withBoundedLocalKv( bounded != 0 ).withKvFp8( kv_fp8 != 0 );
    return mc;
}

/// GemmaModel::fromPretrained( path, GemmaModelConfig( context ).withWeightQuantization( policy ) ): geometry from the artifact's metadata
HOST_API void* mila_gemma_model_from_pretrained( const char* path, int policy, int64_t context, int64_t prefill_chunk, int bounded_local_kv, int device )
{
    RocmGemmaModel* m = nullptr;
    int rc = guarded( [&] { m = RocmGemmaModel::fromPretrained( path, model_config_of( policy, context, prefill_chunk, bounded_local_kv, 0 ), Compute::Device::Rocm( device ) ).release(); } );
    return rc == 0 ? m : nullptr;
}
/// ... with the KV policy switch: kv_fp8 != 0 = GemmaModelConfig::withKvFp8( true )
HOST_API void* mila_gemma_model_from_pretrained_kv( const char* path, int policy, int64_t context, int64_t prefill_chunk, int bounded_local_kv, int kv_fp8, int device )
{
    RocmGemmaModel* m = nullptr;
    int rc = guarded( [&] { m = RocmGemmaModel::fromPretrained( path, model_config_of( policy, context, prefill_chunk, bounded_local_kv, kv_fp8 ), Compute::Device::Rocm( device ) ).release(); } );
    return rc == 0 ? m : nullptr;
}

/// the same model over synthetic parameters; profile as in mila_gemma_init_synthetic (NULL = unit profile)
HOST_API void* mila_gemma_model_synthetic( int policy, const mila_gemma_config* c, int64_t context, int64_t prefill_chunk, uint64_t seed, const float* p, int device )
{
    RocmGemmaModel* m = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg;
        int bounded = 0, kv_fp8 = 0;
        if ( c )
        {
            cfg.vocab_size = c->vocab_size; cfg.embedding_dim = c->embedding_dim; cfg.num_layers = c->num_layers; cfg.num_heads = c->num_heads;
            cfg.num_kv_heads = c->num_kv_heads; cfg.head_dim = c->head_dim; cfg.hidden_dim = c->hidden_dim; cfg.global_head_dim = c->global_head_dim;
            cfg.num_global_kv_heads = c->num_global_kv_heads; cfg.window = c->window; cfg.sliding_window_pattern = c->sliding_window_pattern;
            cfg.global_rotary_dim = c->global_rotary_dim;
            bounded = c->bounded_local_kv != 0;
            kv_fp8 = c->kv_fp8 != 0;
        }
        GemmaTransformer<NoWeightQuant>::SyntheticProfile pr;
        if ( p ) { pr.linear_gain = p[ 0 ]; pr.qk_norm_center = p[ 1 ]; pr.post_norm_center = p[ 2 ]; pr.layer_scalar = p[ 3 ]; pr.table_gain = p[ 4 ]; }
        m = RocmGemmaModel::fromSynthetic( cfg, model_config_of( policy, context, prefill_chunk, bounded, kv_fp8 ), seed, pr, Compute::Device::Rocm( device ) ).release();
    } );
    return rc == 0 ? m : nullptr;
}

/// mila_gemma_model_synthetic with GemmaModelConfig::withMaxBatch( max_batch ): a model generate_rows can run on
HOST_API void* mila_gemma_model_synthetic_rows( int policy, const mila_gemma_config* c, int64_t context, int64_t prefill_chunk, int64_t max_batch, uint64_t seed, const float* p, int device )
{
    RocmGemmaModel* m = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg;
        int bounded = 0, kv_fp8 = 0;
        if ( c )
        {
            cfg.vocab_size = c->vocab_size; cfg.embedding_dim = c->embedding_dim; cfg.num_layers = c->num_layers; cfg.num_heads = c->num_heads;
            cfg.num_kv_heads = c->num_kv_heads; cfg.head_dim = c->head_dim; cfg.hidden_dim = c->hidden_dim; cfg.global_head_dim = c->global_head_dim;
            cfg.num_global_kv_heads = c->num_global_kv_heads; cfg.window = c->window; cfg.sliding_window_pattern = c->sliding_window_pattern;
            cfg.global_rotary_dim = c->global_rotary_dim;
            bounded = c->bounded_local_kv != 0;
            kv_fp8 = c->kv_fp8 != 0;
        }
        GemmaTransformer<NoWeightQuant>::SyntheticProfile pr;
        if ( p ) { pr.linear_gain = p[ 0 ]; pr.qk_norm_center = p[ 1 ]; pr.post_norm_center = p[ 2 ]; pr.layer_scalar = p[ 3 ]; pr.table_gain = p[ 4 ]; }
        m = RocmGemmaModel::fromSynthetic( cfg, model_config_of( policy, context, prefill_chunk, bounded, kv_fp8 ).withMaxBatch( max_batch ), seed, pr, Compute::Device::Rocm( device ) ).release();
    } );
    return rc == 0 ? m : nullptr;
}

/// mila_gemma_model_synthetic_rows with GemmaModelConfig::withKvFp8Rows( kv_fp8_rows != 0 ): the rows model over FP8 KV caches
HOST_API void* mila_gemma_model_synthetic_rows_kv( int policy, const mila_gemma_config* c, int64_t context, int64_t prefill_chunk, int64_t max_batch, int kv_fp8_rows, uint64_t seed,
                                                   const float* p, int device )
{
    RocmGemmaModel* m = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg = gemma_config_of( c );
        GemmaTransformer<NoWeightQuant>::SyntheticProfile pr;
        if ( p ) { pr.linear_gain = p[ 0 ]; pr.qk_norm_center = p[ 1 ]; pr.post_norm_center = p[ 2 ]; pr.layer_scalar = p[ 3 ]; pr.table_gain = p[ 4 ]; }
        m = RocmGemmaModel::fromSynthetic( cfg, model_config_of( policy, context, prefill_chunk, cfg.bounded_local_kv, cfg.kv_fp8 ).withMaxBatch( max_batch ).withKvFp8Rows( kv_fp8_rows != 0 ),
                                           seed, pr, Compute::Device::Rocm( device ) ).release();
    } );
    return rc == 0 ? m : nullptr;
}

/// mila_gemma_model_synthetic_rows with GemmaModelConfig::withBoundedLocalKvRows( bounded_local_kv_rows != 0 ): the rows model with rings on the sliding-window layers
HOST_API void* mila_gemma_model_synthetic_rows_ring( int policy, const mila_gemma_config* c, int64_t context, int64_t prefill_chunk, int64_t max_batch, int bounded_local_kv_rows,
                                                     uint64_t seed, const float* p, int device )
{
    RocmGemmaModel* m = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg = gemma_config_of( c );
        GemmaTransformer<NoWeightQuant>::SyntheticProfile pr;
        if ( p ) { pr.linear_gain = p[ 0 ]; pr.qk_norm_center = p[ 1 ]; pr.post_norm_center = p[ 2 ]; pr.layer_scalar = p[ 3 ]; pr.table_gain = p[ 4 ]; }
        m = RocmGemmaModel::fromSynthetic( cfg, model_config_of( policy, context, prefill_chunk, cfg.bounded_local_kv, cfg.kv_fp8 ).withMaxBatch( max_batch )
                                                    .withBoundedLocalKvRows( bounded_local_kv_rows != 0 ), seed, pr, Compute::Device::Rocm( device ) ).release();
    } );
    return rc == 0 ? m : nullptr;
}

/// mila_gemma_model_synthetic with GemmaModelConfig::withDraftTokens( draft_tokens ): greedy generate() verifies up to draft_tokens drafted tokens per step
HOST_API void* mila_gemma_model_synthetic_chain( int policy, const mila_gemma_config* c, int64_t context, int64_t prefill_chunk, int64_t draft_tokens, uint64_t seed, const float* p, int device )
{
    RocmGemmaModel* m = nullptr;
    int rc = guarded( [&]
    {
        GemmaConfig cfg = gemma_config_of( c );
        GemmaTransformer<NoWeightQuant>::SyntheticProfile pr;
        if ( p ) { pr.linear_gain = p[ 0 ]; pr.qk_norm_center = p[ 1 ]; pr.post_norm_center = p[ 2 ]; pr.layer_scalar = p[ 3 ]; pr.table_gain = p[ 4 ]; }
        m = RocmGemmaModel::fromSynthetic( cfg, model_config_of( policy, context, prefill_chunk, cfg.bounded_local_kv, cfg.kv_fp8 ).withDraftTokens( draft_tokens ), seed, pr,
                                           Compute::Device::Rocm( device ) ).release();
    } );
    return rc == 0 ? m : nullptr;
}

HOST_API void mila_gemma_model_destroy( void* h ) { delete static_cast<RocmGemmaModel*>( h ); }

/// GemmaModel::score: out_logprob [n - first]; out_argmax / out_argmax_logprob [n - first] or both NULL (ScoreParams::argmax off); *out_sum = the float64 sum;
/// *out_reused = tokens served from the KV caches
HOST_API int mila_gemma_model_score( void* h, const int32_t* tokens, int64_t n, int64_t first, float* out_logprob, int32_t* out_argmax, float* out_argmax_logprob,
                                     double* out_sum, int64_t* out_reused )
{
    auto* m = static_cast<RocmGemmaModel*>( h );
    return guarded( [&]
    {
        if ( n < 0 || ( n > 0 && !tokens ) ) throw std::invalid_argument( "model_score: tokens are required" );
        if ( ( out_argmax == nullptr ) != ( out_argmax_logprob == nullptr ) ) throw std::invalid_argument( "model_score: the two argmax outputs go together" );
        ScoreParams sp;
        sp.first = first;
        sp.argmax = out_argmax != nullptr;
        const ScoreResult res = m->score( std::span<const int32_t>( tokens, static_cast<size_t>( n ) ), sp );
        if ( out_logprob ) std::copy( res.logprob.begin(), res.logprob.end(), out_logprob );
        if ( out_argmax ) { std::copy( res.argmax.begin(), res.argmax.end(), out_argmax ); std::copy( res.argmax_logprob.begin(), res.argmax_logprob.end(), out_argmax_logprob ); }
        if ( out_sum ) *out_sum = res.sum;
        if ( out_reused ) *out_reused = m->lastReusedPrefix();
    } );
}

/// generate(): max_new < 0 = no budget (run to a stop token or the context bound); n_stop == 0 = the model's default stop set; the callback's tokens
/// are appended to out_tokens (at most cap).  *out_status = GenerateStatus; *out_reused = prompt tokens served from the KV caches; cancel_after >= 0: the
/// client's stop request is raised from inside on_token once that many tokens were delivered (the std::stop_token of the reference's generate)
/// where the *_logprobs entries collect GenerateParams::on_logprobs: entry i (of one row) goes to logprob[ i ], ids / logprobs[ i * top_n .. ), at most cap entries;
/// top_n < 0 = the request carries no log-probabilities
/// GenerateParams::sampling's filters from filters[4] = min_p, repetition_penalty, presence_penalty, frequency_penalty (NULL: neutral) -- the *_filtered entries below
static void apply_request_filters( decltype( GenerateParams::sampling )& sp, const float* filters )
{
    if ( !filters ) return;
    sp.min_p = filters[ 0 ]; sp.repetition_penalty = filters[ 1 ]; sp.presence_penalty = filters[ 2 ]; sp.frequency_penalty = filters[ 3 ];
}

/// GenerateParams::logit_bias / banned_tokens / allowed_tokens / min_tokens of the *_biased entries below, by pointer (NULL: none of them)
struct mila_token_bias_request
{
    const int32_t* bias_ids; const float* bias_values; int64_t n_bias;      ///< logit_bias: id -> value
    const int32_t* banned; int64_t n_banned;
    const int32_t* allowed; int64_t n_allowed;
    int32_t min_tokens;
};
static void apply_request_bias( GenerateParams& gp, const mila_token_bias_request* b )
{
    if ( !b ) return;
    if ( b->n_bias < 0 || b->n_banned < 0 || b->n_allowed < 0 || ( b->n_bias && ( !b->bias_ids || !b->bias_values ) ) || ( b->n_banned && !b->banned ) || ( b->n_allowed && !b->allowed ) )
        throw std::invalid_argument( "token bias request: null list" );
    for ( int64_t i = 0; i < b->n_bias; ++i ) gp.logit_bias.emplace_back( b->bias_ids[ i ], b->bias_values[ i ] );
    gp.banned_tokens.assign( b->banned, b->banned + b->n_banned );
    gp.allowed_tokens.assign( b->allowed, b->allowed + b->n_allowed );
    gp.min_tokens = b->min_tokens;
}

/// GenerateParams::automaton of the *_automaton entries below, by pointer (NULL: none)
struct mila_token_automaton_request
{
    const uint16_t* class_of; int64_t vocab;      ///< token id -> class
    const uint16_t* next;                         ///< [num_states * num_classes], 0xFFFF = forbidden
    int32_t num_states, num_classes, start;
};
static void apply_request_automaton( GenerateParams& gp, const mila_token_automaton_request* a )
{
    if ( !a ) return;
    if ( !a->class_of || !a->next || a->vocab < 0 || a->num_states < 0 || a->num_classes < 0 ) throw std::invalid_argument( "token automaton request: null table or negative size" );
    auto t = std::make_shared<TokenAutomaton>();
    t->num_states = a->num_states; t->num_classes = a->num_classes; t->start = a->start;
    t->class_of.assign( a->class_of, a->class_of + a->vocab );
    t->next.assign( a->next, a->next + static_cast<size_t>( a->num_states ) * static_cast<size_t>( a->num_classes ) );
    gp.automaton = std::move( t );
}

struct LogprobSink
{
    int top_n{ -1 };
    float* logprob{ nullptr };
    int32_t* ids{ nullptr };
    float* logprobs{ nullptr };
    int64_t cap{ 0 };
    /// sets the request's fields; `count` = entries of this row so far, advanced by the callback
    void attach( GenerateParams& gp, std::function<int64_t&( int )> count )
    {
        if ( top_n < 0 ) return;
        gp.logprobs = top_n;
        gp.on_logprobs = [this, count]( const TokenLogprobs& t )
        {
            int64_t& c = count( t.row );
            const int64_t at = static_cast<int64_t>( t.row ) * cap + c;
            if ( c < cap )
            {
                if ( logprob ) logprob[ at ] = t.logprob;
                for ( size_t i = 0; i < t.top_ids.size(); ++i )
                {
                    if ( ids ) ids[ at * top_n + static_cast<int64_t>( i ) ] = t.top_ids[ i ];
                    if ( logprobs ) logprobs[ at * top_n + static_cast<int64_t>( i ) ] = t.top_logprobs[ i ];
                }
            }
            ++c;
        };
    }
};

static int model_generate_impl( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature, int top_k,
                                float top_p, int64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_reused,
                                int64_t cancel_after, LogprobSink sink, int64_t* out_logprob_count, const float* filters = nullptr, const mila_token_bias_request* bias = nullptr,
                                const mila_token_automaton_request* automaton = nullptr );
HOST_API int mila_gemma_model_generate( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature, int top_k,
                                        float top_p, int64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_reused,
                                        int64_t cancel_after )
{
    return model_generate_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, out_tokens, cap, out_count, out_status, out_reused, cancel_after,
                                LogprobSink{}, nullptr );
}
/// mila_gemma_model_generate with GenerateParams::logprobs = top_n: entry i of on_logprobs goes to out_logprob[ i ] and out_ids / out_logprobs[ i * top_n .. ) (at most
/// cap entries), their number to *out_logprob_count
HOST_API int mila_gemma_model_generate_logprobs( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature, int top_k,
                                                 float top_p, int64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_reused,
                                                 int64_t cancel_after, int top_n, float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_count )
{
    return model_generate_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, out_tokens, cap, out_count, out_status, out_reused, cancel_after,
                                LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_count );
}
/// mila_gemma_model_generate_logprobs with the sampling filters: filters[4] = min_p, repetition_penalty, presence_penalty, frequency_penalty; top_n < 0 = no log-probabilities
HOST_API int mila_gemma_model_generate_filtered( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature, int top_k,
                                                 float top_p, int64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_reused,
                                                 int64_t cancel_after, int top_n, float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_count,
                                                 const float* filters )
{
    if ( !filters ) { g_err = "invalid_argument: gemma_model_generate_filtered: null filters"; return MILA_E_INVALID_ARGUMENT; }
    return model_generate_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, out_tokens, cap, out_count, out_status, out_reused, cancel_after,
                                LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_count, filters );
}
/// mila_gemma_model_generate_filtered (filters may be NULL: neutral) with the bias request (NULL: none)
HOST_API int mila_gemma_model_generate_biased( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature, int top_k,
                                               float top_p, int64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_reused,
                                               int64_t cancel_after, int top_n, float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_count,
                                               const float* filters, const mila_token_bias_request* bias )
{
    return model_generate_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, out_tokens, cap, out_count, out_status, out_reused, cancel_after,
                                LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_count, filters, bias );
}
/// mila_gemma_model_generate_biased (filters and bias may be NULL) with the automaton request (NULL: none)
HOST_API int mila_gemma_model_generate_automaton( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature, int top_k,
                                                  float top_p, int64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_reused,
                                                  int64_t cancel_after, int top_n, float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_count,
                                                  const float* filters, const mila_token_bias_request* bias, const mila_token_automaton_request* automaton )
{
    return model_generate_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, out_tokens, cap, out_count, out_status, out_reused, cancel_after,
                                LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_count, filters, bias, automaton );
}
/// GemmaModel::lastAutomatonState(): *out_has = whether the last generate() had an automaton, *out_state = the state it ended in
HOST_API int mila_gemma_model_last_automaton_state( void* h, int32_t* out_state, int32_t* out_has )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m ) throw std::invalid_argument( "null model" );
        const auto st = m->lastAutomatonState();
        if ( out_has ) *out_has = st ? 1 : 0;
        if ( out_state ) *out_state = st.value_or( -1 );
    } );
}
static int model_generate_impl( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature, int top_k,
                                float top_p, int64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_reused,
                                int64_t cancel_after, LogprobSink sink, int64_t* out_logprob_count, const float* filters, const mila_token_bias_request* bias,
                                const mila_token_automaton_request* automaton )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m || !prompt || !out_count || !out_status ) throw std::invalid_argument( "gemma_model_generate: null argument" );
        GenerateParams gp;
        int64_t n_lp = 0;
        sink.attach( gp, [&]( int ) -> int64_t& { return n_lp; } );
        struct Report { int64_t* out; int64_t& n; ~Report() { if ( out ) *out = n; } } report{ out_logprob_count, n_lp };
        if ( max_new >= 0 ) gp.max_new_tokens = max_new;
        gp.sampling.temperature = temperature; gp.sampling.top_k = top_k; gp.sampling.top_p = top_p;
        apply_request_filters( gp.sampling, filters );
        apply_request_bias( gp, bias );
        apply_request_automaton( gp, automaton );
        for ( int i = 0; i < n_stop; ++i ) gp.stop_tokens.push_back( stop_tokens[ i ] );
        if ( seed >= 0 ) m->seedSampler( static_cast<uint64_t>( seed ) );
        int64_t n = 0;
        std::atomic<bool> stop{ cancel_after == 0 };
        const GenerateStatus st = m->generate( std::span<const int32_t>( prompt, static_cast<size_t>( n_prompt ) ),
                                               [&]( int32_t t ) { if ( out_tokens && n < cap ) out_tokens[ n ] = t; ++n; if ( cancel_after >= 0 && n >= cancel_after ) stop.store( true ); }, gp, &stop );
        *out_count = n;
        *out_status = static_cast<int32_t>( st );
        if ( out_reused ) *out_reused = m->lastReusedPrefix();
    } );
}

/// mila_gemma_model_generate with a drafter for the speculative greedy loop: hint (n_hint > 0) = a sequence the drafter reads the continuation from -- the tokens
/// expected to follow the prompt, so that the draft for the token at index i of the output is hint[ i + 1 .. ]; n_hint == 0 = the default drafter (prompt lookup).
/// out_stats (may be NULL): GemmaModel::lastSpeculation() as { steps, chain_steps, drafted, accepted }
static int generate_spec_impl( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature, int top_k,
                               float top_p, int64_t seed, const int32_t* hint, int64_t n_hint, int speculative_sampling, int32_t* out_tokens, int64_t cap, int64_t* out_count,
                               int32_t* out_status, int64_t* out_stats, LogprobSink sink = LogprobSink{}, int64_t* out_logprob_count = nullptr, const float* filters = nullptr,
                               const mila_token_bias_request* bias = nullptr, const mila_token_automaton_request* automaton = nullptr, int speculate_constrained = 0 )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m || !prompt || !out_count || !out_status ) throw std::invalid_argument( "gemma_model_generate_spec: null argument" );
        GenerateParams gp;
        int64_t n_lp = 0;
        sink.attach( gp, [&]( int ) -> int64_t& { return n_lp; } );
        struct Report { int64_t* out; int64_t& n; ~Report() { if ( out ) *out = n; } } report{ out_logprob_count, n_lp };
        gp.speculative_sampling = speculative_sampling != 0;
        gp.speculate_constrained = speculate_constrained != 0;
        if ( max_new >= 0 ) gp.max_new_tokens = max_new;
        gp.sampling.temperature = temperature; gp.sampling.top_k = top_k; gp.sampling.top_p = top_p;
        apply_request_filters( gp.sampling, filters );
        apply_request_bias( gp, bias );
        apply_request_automaton( gp, automaton );
        for ( int i = 0; i < n_stop; ++i ) gp.stop_tokens.push_back( stop_tokens[ i ] );
        if ( hint && n_hint > 0 )
            gp.draft = [=]( std::span<const int32_t> history, int k )
            {
                // history = prompt + emitted tokens; the tokens after its last element are hint[ emitted .. ]
                const int64_t first = static_cast<int64_t>( history.size() ) - n_prompt;
                std::vector<int32_t> d;
                for ( int64_t i = first; i >= 0 && i < n_hint && static_cast<int>( d.size() ) < k; ++i ) d.push_back( hint[ i ] );
                return d;
            };
        if ( seed >= 0 ) m->seedSampler( static_cast<uint64_t>( seed ) );
        int64_t n = 0;
        const GenerateStatus st = m->generate( std::span<const int32_t>( prompt, static_cast<size_t>( n_prompt ) ), [&]( int32_t t ) { if ( out_tokens && n < cap ) out_tokens[ n ] = t; ++n; }, gp );
        *out_count = n;
        *out_status = static_cast<int32_t>( st );
        if ( out_stats )
        {
            const auto& sp = m->lastSpeculation();
            out_stats[ 0 ] = (int64_t)sp.steps; out_stats[ 1 ] = (int64_t)sp.chain_steps; out_stats[ 2 ] = (int64_t)sp.drafted; out_stats[ 3 ] = (int64_t)sp.accepted;
        }
    } );
}

HOST_API int mila_gemma_model_generate_spec( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature, int top_k,
                                             float top_p, int64_t seed, const int32_t* hint, int64_t n_hint, int32_t* out_tokens, int64_t cap, int64_t* out_count, int32_t* out_status,
                                             int64_t* out_stats )
{
    return generate_spec_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, hint, n_hint, 0, out_tokens, cap, out_count, out_status, out_stats );
}
/// mila_gemma_model_generate_spec with GenerateParams::speculative_sampling: a stochastic request takes the speculative loop too (coupled draws)
HOST_API int mila_gemma_model_generate_spec_sampling( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature,
                                                      int top_k, float top_p, int64_t seed, const int32_t* hint, int64_t n_hint, int speculative_sampling, int32_t* out_tokens,
                                                      int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_stats )
{
    return generate_spec_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, hint, n_hint, speculative_sampling, out_tokens, cap, out_count,
                               out_status, out_stats );
}

/// mila_gemma_model_generate_spec_sampling with GenerateParams::logprobs = top_n; the outputs as in mila_gemma_model_generate_logprobs
HOST_API int mila_gemma_model_generate_spec_logprobs( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature,
                                                      int top_k, float top_p, int64_t seed, const int32_t* hint, int64_t n_hint, int speculative_sampling, int32_t* out_tokens,
                                                      int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_stats, int top_n, float* out_logprob, int32_t* out_ids,
                                                      float* out_logprobs, int64_t* out_logprob_count )
{
    return generate_spec_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, hint, n_hint, speculative_sampling, out_tokens, cap, out_count,
                               out_status, out_stats, LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_count );
}

/// mila_gemma_model_generate_spec_logprobs with the sampling filters (as mila_gemma_model_generate_filtered): a request with any of them set takes the plain loop
HOST_API int mila_gemma_model_generate_spec_filtered( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature,
                                                      int top_k, float top_p, int64_t seed, const int32_t* hint, int64_t n_hint, int speculative_sampling, int32_t* out_tokens,
                                                      int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_stats, int top_n, float* out_logprob, int32_t* out_ids,
                                                      float* out_logprobs, int64_t* out_logprob_count, const float* filters )
{
    if ( !filters ) { g_err = "invalid_argument: gemma_model_generate_spec_filtered: null filters"; return MILA_E_INVALID_ARGUMENT; }
    return generate_spec_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, hint, n_hint, speculative_sampling, out_tokens, cap, out_count,
                               out_status, out_stats, LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_count, filters );
}

/// mila_gemma_model_generate_spec_filtered (filters may be NULL) with the bias request (NULL: none): a request with a bias takes the plain loop
HOST_API int mila_gemma_model_generate_spec_biased( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature,
                                                    int top_k, float top_p, int64_t seed, const int32_t* hint, int64_t n_hint, int speculative_sampling, int32_t* out_tokens,
                                                    int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_stats, int top_n, float* out_logprob, int32_t* out_ids,
                                                    float* out_logprobs, int64_t* out_logprob_count, const float* filters, const mila_token_bias_request* bias )
{
    return generate_spec_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, hint, n_hint, speculative_sampling, out_tokens, cap, out_count,
                               out_status, out_stats, LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_count, filters, bias );
}

/// mila_gemma_model_generate_spec_biased with the automaton request (NULL: none): a constrained request takes the plain loop
HOST_API int mila_gemma_model_generate_spec_automaton( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature,
                                                       int top_k, float top_p, int64_t seed, const int32_t* hint, int64_t n_hint, int speculative_sampling, int32_t* out_tokens,
                                                       int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_stats, int top_n, float* out_logprob, int32_t* out_ids,
                                                       float* out_logprobs, int64_t* out_logprob_count, const float* filters, const mila_token_bias_request* bias,
                                                       const mila_token_automaton_request* automaton )
{
    return generate_spec_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, hint, n_hint, speculative_sampling, out_tokens, cap, out_count,
                               out_status, out_stats, LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_count, filters, bias, automaton );
}

/// mila_gemma_model_generate_spec_automaton with GenerateParams::speculate_constrained: with it set, a request with a bias and / or an automaton takes the speculative loop
HOST_API int mila_gemma_model_generate_spec_constrained( void* h, const int32_t* prompt, int64_t n_prompt, int max_new, const int32_t* stop_tokens, int n_stop, float temperature,
                                                         int top_k, float top_p, int64_t seed, const int32_t* hint, int64_t n_hint, int speculative_sampling, int32_t* out_tokens,
                                                         int64_t cap, int64_t* out_count, int32_t* out_status, int64_t* out_stats, int top_n, float* out_logprob, int32_t* out_ids,
                                                         float* out_logprobs, int64_t* out_logprob_count, const float* filters, const mila_token_bias_request* bias,
                                                         const mila_token_automaton_request* automaton, int speculate_constrained )
{
    return generate_spec_impl( h, prompt, n_prompt, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, hint, n_hint, speculative_sampling, out_tokens, cap, out_count,
                               out_status, out_stats, LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_count, filters, bias, automaton,
                               speculate_constrained );
}

/// TokenAutomaton::forcedTokens under a table that bans `banned` (n_banned may be 0): out[ num_states ] = the one token a state allows, else -1.  Host only.
HOST_API int mila_token_automaton_forced_tokens( const mila_token_automaton_request* automaton, const int32_t* banned, int64_t n_banned, int32_t* out )
{
    return guarded( [&]
    {
        if ( !automaton || !out || n_banned < 0 || ( n_banned && !banned ) ) throw std::invalid_argument( "token_automaton_forced_tokens: null argument" );
        GenerateParams gp;
        apply_request_automaton( gp, automaton );
        gp.automaton->validate( automaton->vocab );
        TokenBiasRequest rq;
        rq.banned_tokens.assign( banned, banned + n_banned );
        const std::vector<int32_t> forced = gp.automaton->forcedTokens( composeTokenBias( rq, automaton->vocab ) );
        std::copy( forced.begin(), forced.end(), out );
    } );
}

/// the vocabulary size of the model (what the ids of a bias request are checked against)
HOST_API int64_t mila_gemma_model_vocab_size( void* h )
{
    auto* m = static_cast<RocmGemmaModel*>( h );
    return m ? static_cast<int64_t>( m->vocabSize() ) : 0;
}

/// GemmaModel::lastSpeculation() as { steps, chain_steps, drafted, accepted }
HOST_API int mila_gemma_model_speculation_stats( void* h, int64_t* out )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m || !out ) throw std::invalid_argument( "gemma_model_speculation_stats: null argument" );
        const auto& sp = m->lastSpeculation();
        out[ 0 ] = (int64_t)sp.steps; out[ 1 ] = (int64_t)sp.chain_steps; out[ 2 ] = (int64_t)sp.drafted; out[ 3 ] = (int64_t)sp.accepted;
    } );
}

/// GemmaModel::lastSpeculation() in full: { steps, chain_steps, drafted, accepted, forced, forced_accepted }
HOST_API int mila_gemma_model_speculation_stats_forced( void* h, int64_t* out )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m || !out ) throw std::invalid_argument( "gemma_model_speculation_stats_forced: null argument" );
        const auto& sp = m->lastSpeculation();
        out[ 0 ] = (int64_t)sp.steps; out[ 1 ] = (int64_t)sp.chain_steps; out[ 2 ] = (int64_t)sp.drafted; out[ 3 ] = (int64_t)sp.accepted;
        out[ 4 ] = (int64_t)sp.forced; out[ 5 ] = (int64_t)sp.forced_accepted;
    } );
}

/// GemmaModel::generateBatch: n_prompts prompts, prompt b = prompts[ offsets[b] .. offsets[b + 1] ); parameters as mila_gemma_model_generate (shared by the rows); seed: row b's
/// generator is seeded seed + b.  Row b's tokens go to out_tokens[ b * cap .. ] (at most cap), their number to out_counts[ b ], its GenerateStatus to out_status[ b ]
static int model_generate_rows_impl( void* h, const int32_t* prompts, const int64_t* offsets, int n_prompts, int max_new, const int32_t* stop_tokens, int n_stop, float temperature,
                                     int top_k, float top_p, uint64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_counts, int32_t* out_status, LogprobSink sink,
                                     int64_t* out_logprob_counts, const float* filters = nullptr, const mila_token_bias_request* bias = nullptr );
HOST_API int mila_gemma_model_generate_rows( void* h, const int32_t* prompts, const int64_t* offsets, int n_prompts, int max_new, const int32_t* stop_tokens, int n_stop, float temperature,
                                             int top_k, float top_p, uint64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_counts, int32_t* out_status )
{
    return model_generate_rows_impl( h, prompts, offsets, n_prompts, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, out_tokens, cap, out_counts, out_status, LogprobSink{},
                                     nullptr );
}
/// mila_gemma_model_generate_rows with GenerateParams::logprobs = top_n: row b's entry i goes to out_logprob[ b * cap + i ] and out_ids / out_logprobs[ (b * cap + i) * top_n .. ),
/// their number to out_logprob_counts[ b ]
HOST_API int mila_gemma_model_generate_rows_logprobs( void* h, const int32_t* prompts, const int64_t* offsets, int n_prompts, int max_new, const int32_t* stop_tokens, int n_stop,
                                                      float temperature, int top_k, float top_p, uint64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_counts, int32_t* out_status,
                                                      int top_n, float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_counts )
{
    return model_generate_rows_impl( h, prompts, offsets, n_prompts, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, out_tokens, cap, out_counts, out_status,
                                     LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_counts );
}
/// mila_gemma_model_generate_rows_logprobs with the sampling filters (as mila_gemma_model_generate_filtered), shared by the rows
HOST_API int mila_gemma_model_generate_rows_filtered( void* h, const int32_t* prompts, const int64_t* offsets, int n_prompts, int max_new, const int32_t* stop_tokens, int n_stop,
                                                      float temperature, int top_k, float top_p, uint64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_counts, int32_t* out_status,
                                                      int top_n, float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_counts, const float* filters )
{
    if ( !filters ) { g_err = "invalid_argument: gemma_model_generate_rows_filtered: null filters"; return MILA_E_INVALID_ARGUMENT; }
    return model_generate_rows_impl( h, prompts, offsets, n_prompts, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, out_tokens, cap, out_counts, out_status,
                                     LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_counts, filters );
}
/// mila_gemma_model_generate_rows_filtered (filters may be NULL) with the bias request (NULL: none), shared by the rows
HOST_API int mila_gemma_model_generate_rows_biased( void* h, const int32_t* prompts, const int64_t* offsets, int n_prompts, int max_new, const int32_t* stop_tokens, int n_stop,
                                                    float temperature, int top_k, float top_p, uint64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_counts, int32_t* out_status,
                                                    int top_n, float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_counts, const float* filters,
                                                    const mila_token_bias_request* bias )
{
    return model_generate_rows_impl( h, prompts, offsets, n_prompts, max_new, stop_tokens, n_stop, temperature, top_k, top_p, seed, out_tokens, cap, out_counts, out_status,
                                     LogprobSink{ top_n, out_logprob, out_ids, out_logprobs, cap }, out_logprob_counts, filters, bias );
}
static int model_generate_rows_impl( void* h, const int32_t* prompts, const int64_t* offsets, int n_prompts, int max_new, const int32_t* stop_tokens, int n_stop, float temperature,
                                     int top_k, float top_p, uint64_t seed, int32_t* out_tokens, int64_t cap, int64_t* out_counts, int32_t* out_status, LogprobSink sink,
                                     int64_t* out_logprob_counts, const float* filters, const mila_token_bias_request* bias )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m || !prompts || !offsets || !out_counts || !out_status || n_prompts < 0 ) throw std::invalid_argument( "gemma_model_generate_rows: null argument" );
        GenerateParams gp;
        std::vector<int64_t> lp_counts( static_cast<size_t>( std::max( n_prompts, 1 ) ), 0 );
        sink.attach( gp, [&]( int b ) -> int64_t& { return lp_counts.at( static_cast<size_t>( b ) ); } );
        if ( max_new >= 0 ) gp.max_new_tokens = max_new;
        gp.sampling.temperature = temperature; gp.sampling.top_k = top_k; gp.sampling.top_p = top_p;
        apply_request_filters( gp.sampling, filters );
        apply_request_bias( gp, bias );
        for ( int i = 0; i < n_stop; ++i ) gp.stop_tokens.push_back( stop_tokens[ i ] );
        std::vector<std::vector<int32_t>> ps;
        for ( int b = 0; b < n_prompts; ++b ) ps.emplace_back( prompts + offsets[ b ], prompts + offsets[ b + 1 ] );
        std::vector<int64_t> counts( static_cast<size_t>( n_prompts ), 0 );
        const auto st = m->generateBatch( ps, [&]( int b, int32_t t ) { int64_t& c = counts[ static_cast<size_t>( b ) ]; if ( out_tokens && c < cap ) out_tokens[ b * cap + c ] = t; ++c; }, gp, seed );
        for ( int b = 0; b < n_prompts; ++b ) { out_counts[ b ] = counts[ static_cast<size_t>( b ) ]; out_status[ b ] = static_cast<int32_t>( st[ static_cast<size_t>( b ) ] ); }
        if ( out_logprob_counts ) for ( int b = 0; b < n_prompts; ++b ) out_logprob_counts[ b ] = lp_counts[ static_cast<size_t>( b ) ];
    } );
}

/// out[0] = captures of the model's rows graph so far, out[1] = kernel nodes of the captured rows step
HOST_API int mila_gemma_model_rows_graph_info( void* h, int64_t* out )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m || !out ) throw std::invalid_argument( "gemma_model_rows_graph_info: null argument" );
        std::visit( [&]( auto& net ) { out[ 0 ] = (int64_t)net->graphRowsCaptureCount(); out[ 1 ] = (int64_t)net->graphRowsNodeCount(); }, m->network() );
    } );
}
/// One row of mila_gemma_model_generate_requests: generate()'s arguments by value and by pointer
struct mila_gemma_row_request
{
    const int32_t* prompt; int64_t n_prompt;
    const int32_t* stop_tokens; int64_t n_stop;
    const mila_token_bias_request* bias;                 ///< NULL: none
    const mila_token_automaton_request* automaton;       ///< NULL: none
    uint64_t seed;
    float temperature, top_p;
    float filters[ 4 ];                                  ///< min_p, repetition_penalty, presence_penalty, frequency_penalty
    int32_t top_k;
    int32_t max_new;                                     ///< < 0: none
    int32_t logprobs;                                    ///< < 0: none
    int32_t speculative;                                 ///< bit 0 speculative_sampling, bit 1 speculate_constrained, bit 2 a drafter: all refused
};
/// the C rows of a requests call as BatchRequests (who: the entry's name for the refusals); the log-probability sink counts per request
static void read_row_requests( const mila_gemma_row_request* requests, int n, std::vector<BatchRequest>& rq, LogprobSink& sink, std::vector<int64_t>& lp_counts, const char* who )
{
    for ( int b = 0; b < n; ++b )
    {
        const auto& q = requests[ b ];
        auto& r = rq[ static_cast<size_t>( b ) ];
        if ( q.n_prompt < 0 || q.n_stop < 0 || ( q.n_prompt && !q.prompt ) || ( q.n_stop && !q.stop_tokens ) ) throw std::invalid_argument( std::string( who ) + ": null list" );
        r.prompt.assign( q.prompt, q.prompt + q.n_prompt );
        r.seed = q.seed;
        GenerateParams& gp = r.params;
        sink.attach( gp, [&lp_counts]( int row ) -> int64_t& { return lp_counts.at( static_cast<size_t>( row ) ); } );
        if ( q.logprobs >= 0 ) gp.logprobs = q.logprobs; else gp.logprobs.reset();      // each row's own value: the model refuses rows that differ
        if ( q.max_new >= 0 ) gp.max_new_tokens = q.max_new;
        gp.sampling.temperature = q.temperature; gp.sampling.top_k = q.top_k; gp.sampling.top_p = q.top_p;
        apply_request_filters( gp.sampling, q.filters );
        apply_request_bias( gp, q.bias );
        apply_request_automaton( gp, q.automaton );
        gp.stop_tokens.assign( q.stop_tokens, q.stop_tokens + q.n_stop );
        gp.speculative_sampling = ( q.speculative & 1 ) != 0;
        gp.speculate_constrained = ( q.speculative & 2 ) != 0;
        if ( q.speculative & 4 ) gp.draft = []( std::span<const int32_t>, int ) { return std::vector<int32_t>{}; };
    }
}
/// GemmaModel::generateRequests: row b runs requests[ b ].  out_tokens [n, cap], out_counts / out_status [n]; the log-probability entries of row b at
/// out_logprob[ b * cap .. ) and out_ids / out_logprobs[ ( b * cap + i ) * top_n .. ) with top_n = requests[ 0 ].logprobs (the arrays may be NULL without
/// log-probabilities), their numbers to out_logprob_counts [n]; out_states / out_has_state [n]: the final automaton state of a row that had one
HOST_API int mila_gemma_model_generate_requests( void* h, const mila_gemma_row_request* requests, int n, int32_t* out_tokens, int64_t cap, int64_t* out_counts, int32_t* out_status,
                                                 float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_counts, int32_t* out_states, int32_t* out_has_state )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m || !requests || !out_counts || !out_status || n < 0 ) throw std::invalid_argument( "gemma_model_generate_requests: null argument" );
        std::vector<BatchRequest> rq( static_cast<size_t>( n ) );
        std::vector<int64_t> lp_counts( static_cast<size_t>( std::max( n, 1 ) ), 0 );
        LogprobSink sink{ n > 0 ? requests[ 0 ].logprobs : -1, out_logprob, out_ids, out_logprobs, cap };
        read_row_requests( requests, n, rq, sink, lp_counts, "gemma_model_generate_requests" );
        std::vector<int64_t> counts( static_cast<size_t>( n ), 0 );
        std::vector<std::optional<int32_t>> states;
        const auto st = m->generateRequests( rq, [&]( int b, int32_t t ) { int64_t& c = counts[ static_cast<size_t>( b ) ]; if ( out_tokens && c < cap ) out_tokens[ b * cap + c ] = t; ++c; }, &states );
        for ( int b = 0; b < n; ++b )
        {
            out_counts[ b ] = counts[ static_cast<size_t>( b ) ]; out_status[ b ] = static_cast<int32_t>( st[ static_cast<size_t>( b ) ] );
            if ( out_logprob_counts ) out_logprob_counts[ b ] = lp_counts[ static_cast<size_t>( b ) ];
            if ( out_states ) out_states[ b ] = states[ static_cast<size_t>( b ) ].value_or( 0 );
            if ( out_has_state ) out_has_state[ b ] = states[ static_cast<size_t>( b ) ] ? 1 : 0;
        }
    } );
}
/// GemmaModel::serveRequests: mila_gemma_model_generate_requests for ANY n >= 1, the outputs indexed by REQUEST.  Beside them: out_rows [n] the row a request ran in,
/// out_admitted_at [n] the rows steps replayed before its admission, out_finish_order [n] the position of its on_finish among the call's, and out_stats [5] =
/// {rows steps, prefills, prefill tokens, forks, rows-graph captures during the call}, out_times [4] = the host milliseconds the call's admissions spent in
/// {the rows' setters, prefills, forks, first samples}
static int serve_requests( void* h, const mila_gemma_row_request* requests, int n, int32_t* out_tokens, int64_t cap, int64_t* out_counts, int32_t* out_status,
                           float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_counts, int32_t* out_states, int32_t* out_has_state,
                           int32_t* out_rows, int64_t* out_admitted_at, int32_t* out_finish_order, int64_t* out_stats, double* out_times,
                           const RocmGemmaModel::ServeParams& serve, int64_t* out_reused, int32_t* out_donor, int64_t* out_prefix_stats )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m || !requests || !out_counts || !out_status || n < 0 ) throw std::invalid_argument( "gemma_model_serve_requests: null argument" );
        std::vector<BatchRequest> rq( static_cast<size_t>( n ) );
        std::vector<int64_t> lp_counts( static_cast<size_t>( std::max( n, 1 ) ), 0 );
        LogprobSink sink{ n > 0 ? requests[ 0 ].logprobs : -1, out_logprob, out_ids, out_logprobs, cap };
        read_row_requests( requests, n, rq, sink, lp_counts, "gemma_model_serve_requests" );
        std::vector<int64_t> counts( static_cast<size_t>( n ), 0 );
        std::vector<int32_t> finished( static_cast<size_t>( n ), -1 );
        int32_t finishes = 0;
        std::vector<std::optional<int32_t>> states;
        RocmGemmaModel::ServeStats stats;
        const auto st = m->serveRequests( rq, [&]( int q, int32_t t ) { int64_t& c = counts[ static_cast<size_t>( q ) ]; if ( out_tokens && c < cap ) out_tokens[ q * cap + c ] = t; ++c; },
                                          serve, [&]( int q, GenerateStatus )
                                          {
                                              if ( finished.at( static_cast<size_t>( q ) ) >= 0 ) throw std::logic_error( "gemma_model_serve_requests: a request finished twice" );
                                              finished[ static_cast<size_t>( q ) ] = finishes++;
                                          }, &states, &stats );
        for ( int q = 0; q < n; ++q )
        {
            const size_t i = static_cast<size_t>( q );
            out_counts[ q ] = counts[ i ]; out_status[ q ] = static_cast<int32_t>( st[ i ] );
            if ( out_logprob_counts ) out_logprob_counts[ q ] = lp_counts[ i ];
            if ( out_states ) out_states[ q ] = states[ i ].value_or( 0 );
            if ( out_has_state ) out_has_state[ q ] = states[ i ] ? 1 : 0;
            if ( out_rows ) out_rows[ q ] = stats.row[ i ];
            if ( out_admitted_at ) out_admitted_at[ q ] = stats.admitted_at[ i ];
            if ( out_finish_order ) out_finish_order[ q ] = finished[ i ];
            if ( out_reused ) out_reused[ q ] = serve.prefix_cache ? stats.reused_tokens[ i ] : 0;
            if ( out_donor ) out_donor[ q ] = serve.prefix_cache ? stats.donor_row[ i ] : -1;
        }
        if ( out_prefix_stats ) { out_prefix_stats[ 0 ] = stats.prefix_forks; out_prefix_stats[ 1 ] = stats.prefix_in_place; }
        if ( out_stats ) { out_stats[ 0 ] = stats.steps; out_stats[ 1 ] = stats.prefills; out_stats[ 2 ] = stats.prefill_tokens; out_stats[ 3 ] = stats.forks; out_stats[ 4 ] = stats.captures; }
        if ( out_times ) { out_times[ 0 ] = stats.setters_ms; out_times[ 1 ] = stats.prefill_ms; out_times[ 2 ] = stats.fork_ms; out_times[ 3 ] = stats.first_sample_ms; }
    } );
}
HOST_API int mila_gemma_model_serve_requests( void* h, const mila_gemma_row_request* requests, int n, int32_t* out_tokens, int64_t cap, int64_t* out_counts, int32_t* out_status,
                                              float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_counts, int32_t* out_states, int32_t* out_has_state,
                                              int32_t* out_rows, int64_t* out_admitted_at, int32_t* out_finish_order, int64_t* out_stats, double* out_times )
{
    return serve_requests( h, requests, n, out_tokens, cap, out_counts, out_status, out_logprob, out_ids, out_logprobs, out_logprob_counts, out_states, out_has_state, out_rows,
                           out_admitted_at, out_finish_order, out_stats, out_times, RocmGemmaModel::ServeParams{}, nullptr, nullptr, nullptr );
}
/// mila_gemma_model_serve_requests with GemmaModel::ServeParams: prefix_cache != 0 turns the prefix cache on, min_prefix is its shortest reused prefix.  Beside the
/// outputs above: out_reused [n] the prompt positions a request did not prefill, out_donor [n] the row they came from (-1: none), out_prefix_stats [2] =
/// {forkRowPrefix calls, in-place reuses}
HOST_API int mila_gemma_model_serve_requests_prefix( void* h, const mila_gemma_row_request* requests, int n, int32_t* out_tokens, int64_t cap, int64_t* out_counts,
                                                     int32_t* out_status, float* out_logprob, int32_t* out_ids, float* out_logprobs, int64_t* out_logprob_counts,
                                                     int32_t* out_states, int32_t* out_has_state, int32_t* out_rows, int64_t* out_admitted_at, int32_t* out_finish_order,
                                                     int64_t* out_stats, double* out_times, int prefix_cache, int min_prefix, int64_t* out_reused, int32_t* out_donor,
                                                     int64_t* out_prefix_stats )
{
    RocmGemmaModel::ServeParams serve;
    serve.prefix_cache = prefix_cache != 0;
    serve.min_prefix = min_prefix;
    return serve_requests( h, requests, n, out_tokens, cap, out_counts, out_status, out_logprob, out_ids, out_logprobs, out_logprob_counts, out_states, out_has_state, out_rows,
                           out_admitted_at, out_finish_order, out_stats, out_times, serve, out_reused, out_donor, out_prefix_stats );
}
/// GemmaModel::clearPrefixCache
HOST_API int mila_gemma_model_clear_prefix_cache( void* h )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m ) throw std::invalid_argument( "gemma_model_clear_prefix_cache: null argument" );
        m->clearPrefixCache();
    } );
}
/// GemmaModel::prefixCacheLengths: out [4], one length per row of the model; *out_rows = the rows
HOST_API int mila_gemma_model_prefix_cache_lengths( void* h, int64_t* out, int32_t* out_rows )
{
    return guarded( [&]
    {
        auto* m = static_cast<RocmGemmaModel*>( h );
        if ( !m || !out || !out_rows ) throw std::invalid_argument( "gemma_model_prefix_cache_lengths: null argument" );
        const auto lengths = m->prefixCacheLengths();
        *out_rows = static_cast<int32_t>( lengths.size() );
        for ( size_t r = 0; r < lengths.size() && r < 4; ++r ) out[ r ] = lengths[ r ];
    } );
}

}  // extern "C"
