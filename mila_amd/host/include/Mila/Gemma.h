// Gemma-4 decoder on the CDNA4 device: GemmaConfig, and GemmaTransformer<TWeightQuant> with
//   * decode()/prefill() in the REFERENCE's per-component order (one C-ABI call per component
//     forward, exactly the sequence of GemmaBlock::decode / ::prefill,
//     /root/reference/Mila/Src/Dnn/Components/Transformers/Gemma/Gemma.Block.ixx:197-356, and
//     GemmaTransformer::decode, Gemma.ixx:281-297), and
//   * decodeFused(): the same arithmetic as 6 launches per layer (7 with GemmaConfig::kv_fp8, the FP8 KV cache), and
//   * a hipGraph of the fused step with the position in device memory (one replay per token).
// The three paths produce bit-identical logits (tests/test_gemma_host_gpu.py).
//
// Quirks kept from the reference (SURVEY.md Appendix A "Gemma block quirks"): sandwich norms; per-head
// q/k/v norms; RoPE after q/k norm and never on V; global layers have no V projection, V =
// v_norm(raw k_proj); residuals use the block input and res1; output scaled by a per-layer scalar;
// embedding scaled by sqrt(D) with a second bf16 rounding; layer i is global iff (i+1) % 6 == 0;
// tied table: bf16 for NoWeightQuant, per-row FP8 for quantized bodies (Gemma.ixx:143-147).
#pragma once
#include <functional>
#include <map>
#include <optional>
#include <span>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>

#include "GemmaBlock.h"
#include "Serialization.h"
#include "TokenAutomaton.h"

namespace Mila::Dnn
{
    struct GemmaConfig
    {
        // defaults = Gemma-4 12B (Gemma.Config.ixx:796-821)
        dim_t vocab_size = 262144, embedding_dim = 3840, num_layers = 48, num_heads = 16, num_kv_heads = 8, head_dim = 256,
              hidden_dim = 15360, global_head_dim = 512, num_global_kv_heads = 1, window = 1024, sliding_window_pattern = 6,
              global_rotary_dim = 128;
        float rms_norm_eps = 1e-6f, rope_theta_local = 10000.0f, rope_theta_global = 1000000.0f, final_logit_softcapping = 30.0f;
        bool bounded_local_kv = false;   ///< SlidingWindowKvCache on the sliding-window layers (ring of window + chunk - 1 rows)
        bool kv_fp8 = false;             ///< PerChannelKvFp8<> on every layer: e4m3 K / V + one fp32 scale per KV head per cached token, (HS + 4) / (2 HS) of the bf16 bytes
        bool kv_fp8_rows = false;        ///< kv_fp8 (implied) that max_batch > 1 may be combined with: one FP8 KV cache per row, the rows step on the FP8 rows entries (two launches per layer)
        bool bounded_local_kv_rows = false;   ///< bounded_local_kv (implied) that max_batch > 1 may be combined with: one ring per row on the sliding-window layers, forks of the live band, a valid-from bound per row
        dim_t max_batch = 1;             ///< independent sequences a decode step can carry (1 .. 4): KV caches, decode buffers, logits and position words per row
        dim_t draft_tokens = 0;          ///< drafted tokens a chain step can verify (0 .. 3): the rows decode buffers for draft_tokens + 1 rows on the ONE cache, no extra caches

        bool isGlobalLayer( dim_t i ) const { return ( i + 1 ) % sliding_window_pattern == 0; }   // Gemma.Config.ixx:504-507
        dim_t headDim( bool g ) const { return g ? global_head_dim : head_dim; }
        dim_t numKvHeads( bool g ) const { return g ? num_global_kv_heads : num_kv_heads; }
        dim_t qWidth( bool g ) const { return num_heads * headDim( g ); }
        dim_t kvWidth( bool g ) const { return numKvHeads( g ) * headDim( g ); }
        dim_t packedQkvWidth( bool g ) const { return qWidth( g ) + ( g ? 1 : 2 ) * kvWidth( g ); }   // K=V on global layers
        dim_t windowFor( bool g ) const { return g ? 0 : window; }
        float embeddingScale() const { return std::sqrt( static_cast<float>( embedding_dim ) ); }
        bool kvFp8() const noexcept { return kv_fp8 || kv_fp8_rows; }      // the FP8 KV cache on every layer, by either switch
        bool boundedLocalKv() const noexcept { return bounded_local_kv || bounded_local_kv_rows; }      // rings on the sliding-window layers, by either switch

        void validate() const
        {
            if ( embedding_dim <= 0 || num_layers <= 0 || num_heads <= 0 || hidden_dim <= 0 || vocab_size <= 0 )
                throw std::invalid_argument( "GemmaConfig: dimensions must be positive" );
            if ( num_heads % num_kv_heads != 0 || num_heads % num_global_kv_heads != 0 )
                throw std::invalid_argument( "GemmaConfig: num_heads must be a multiple of the KV head counts" );
            if ( embedding_dim % 128 != 0 || hidden_dim % 128 != 0 || qWidth( false ) % 128 != 0 || qWidth( true ) % 128 != 0 )
                throw std::invalid_argument( "GemmaConfig: feature widths must be multiples of 128 (FP4 group size)" );
            if ( max_batch < 1 || max_batch > 4 )
                throw std::invalid_argument( "GemmaConfig: max_batch " + std::to_string( max_batch ) + " outside 1 .. 4 (the rows kernels keep every row's x in LDS)" );
            if ( max_batch > 1 && kv_fp8 && !kv_fp8_rows ) throw std::invalid_argument( "GemmaConfig: max_batch > 1 cannot be combined with kv_fp8 (the FP8 KV cache's fused append is B = 1)" );
            if ( max_batch > 1 && bounded_local_kv && !bounded_local_kv_rows ) throw std::invalid_argument( "GemmaConfig: max_batch > 1 cannot be combined with bounded_local_kv (the ring needs a rewind rule per row)" );
            if ( bounded_local_kv_rows )
            {
                if ( kvFp8() ) throw std::invalid_argument( "GemmaConfig: bounded_local_kv_rows cannot be combined with kv_fp8 (the FP8 KV cache is unbounded; FP8 rings are not built)" );
                if ( draft_tokens > 0 )
                    throw std::invalid_argument( "GemmaConfig: bounded_local_kv_rows cannot be combined with draft_tokens > 0 (rejected drafts leave stale rows, and a ring may already have evicted what they overwrote)" );
                if ( window <= 0 ) throw std::invalid_argument( "GemmaConfig: bounded_local_kv_rows needs a sliding window (window " + std::to_string( window ) + ")" );
            }
            if ( draft_tokens < 0 || draft_tokens > 3 )
                throw std::invalid_argument( "GemmaConfig: draft_tokens " + std::to_string( draft_tokens ) + " outside 0 .. 3 (a chain step is the last token plus the drafts: at most the four rows of the rows kernels)" );
            if ( draft_tokens > 0 )
            {
                if ( max_batch > 1 )
                    throw std::invalid_argument( "GemmaConfig: draft_tokens > 0 cannot be combined with max_batch > 1 (a chain step's rows are consecutive positions of ONE sequence on one cache; "
                                                 "the rows of a batched step are independent sequences, and the two share the four rows of the rows kernels)" );
                if ( kvFp8() ) throw std::invalid_argument( "GemmaConfig: draft_tokens > 0 cannot be combined with kv_fp8 (the FP8 KV cache's fused append is B = 1; the chain over it is not built)" );
                if ( bounded_local_kv )
                    throw std::invalid_argument( "GemmaConfig: draft_tokens > 0 cannot be combined with bounded_local_kv (rejected drafts leave stale rows, and a ring may already have evicted what they overwrote)" );
                for ( dim_t hs : { head_dim, global_head_dim } )
                    if ( hs != 64 && hs != 128 && hs != 256 && hs != 512 )
                        throw std::invalid_argument( "GemmaConfig: draft_tokens > 0 needs head dimensions of 64, 128, 256 or 512 (head_dim " + std::to_string( head_dim ) + ", global_head_dim " +
                                                     std::to_string( global_head_dim ) + ")" );
            }
            if ( kvFp8() )
            {
                if ( bounded_local_kv ) throw std::invalid_argument( "GemmaConfig: kv_fp8 cannot be combined with bounded_local_kv (the FP8 KV cache is unbounded)" );
                for ( dim_t hs : { head_dim, global_head_dim } )
                    if ( hs != 64 && hs != 128 && hs != 256 && hs != 512 )
                        throw std::invalid_argument( "GemmaConfig: kv_fp8 needs head dimensions of 64, 128, 256 or 512 (head_dim " + std::to_string( head_dim ) + ", global_head_dim " +
                                                     std::to_string( global_head_dim ) + ")" );
            }
        }

        /// weight parameters streamed per decode token (Linear body, tied table) -- SURVEY.md section 8d
        dim_t linearParamsPerLayer( bool g ) const
        {
            return embedding_dim * packedQkvWidth( g ) + qWidth( g ) * embedding_dim + embedding_dim * 2 * hidden_dim + hidden_dim * embedding_dim;
        }
    };

    inline void hipCheck( hipError_t e, const char* what )
    {
        if ( e != hipSuccess ) throw Compute::RocmException( std::string( what ) + ": " + hipGetErrorString( e ) );
    }

    template<WeightQuantPolicy TWeightQuant>
    class GemmaTransformer
    {
    public:
        static constexpr DeviceType kDevice = DeviceType::Rocm;
        static constexpr TensorDataType kPrecision = TensorDataType::BF16;
        using TensorType = Tensor<kPrecision, Compute::RocmDeviceMemoryResource>;
        using TokenTensor = Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>;
        using LogitsTensor = Tensor<TensorDataType::FP32, Compute::RocmDeviceMemoryResource>;
        using LinearType = Linear<kDevice, kPrecision, TWeightQuant>;
        using TableQuantizationPolicy = std::conditional_t<TWeightQuant::kIsQuantized, Quant::Weight::PerChannelFp8<>, NoWeightQuant>;
        using LmHeadLinearType = Linear<kDevice, kPrecision, TableQuantizationPolicy>;
        using RmsNormType = RmsNorm<kDevice, kPrecision>;
        using TokenEmbeddingType = TokenEmbedding<kDevice, TensorDataType::INT32, kPrecision, TableQuantizationPolicy>;
        // Gemma.ixx:153-154: local blocks take the model's KV policy, global blocks attend to the whole context
        using LocalBlockType = GemmaBlock<kDevice, kPrecision, false, TWeightQuant, Quant::KvCache::NoKvCompression>;
        using BoundedLocalBlockType = GemmaBlock<kDevice, kPrecision, false, TWeightQuant, Quant::KvCache::SlidingWindowKvCache>;
        using GlobalBlockType = GemmaBlock<kDevice, kPrecision, true, TWeightQuant, Quant::KvCache::NoKvCompression>;
        // ... and with GemmaConfig::kv_fp8 every block keeps its K / V in the FP8 KV cache (unbounded on both kinds)
        using KvFp8LocalBlockType = GemmaBlock<kDevice, kPrecision, false, TWeightQuant, Quant::KvCache::PerChannelKvFp8<>>;
        using KvFp8GlobalBlockType = GemmaBlock<kDevice, kPrecision, true, TWeightQuant, Quant::KvCache::PerChannelKvFp8<>>;
        static constexpr int kFmt = Quant::Weight::abiWeightFormat<TWeightQuant>();
        static constexpr int kTableFmt = Quant::Weight::abiWeightFormat<TableQuantizationPolicy>();

        /// a block behind its kind-independent face: the children (input_norm ... fc_down, rope, res_1/2, geglu), layer_scalar, the KV
        /// cache surface, and IDecoderLayer's prefill / decode (the reference-order path)
        using Layer = GemmaBlockBase<kDevice, kPrecision, TWeightQuant>;
        /// the model's blocks, indexed and iterated as Layer&
        class LayerList
        {
        public:
            using Store = std::vector<std::shared_ptr<Layer>>;
            struct Iterator
            {
                typename Store::const_iterator p;
                Layer& operator*() const { return **p; }
                Iterator& operator++() { ++p; return *this; }
                bool operator!=( const Iterator& o ) const { return p != o.p; }
            };
            size_t size() const noexcept { return v_.size(); }
            Layer& operator[]( size_t i ) const { return *v_[ i ]; }
            Iterator begin() const { return Iterator{ v_.begin() }; }
            Iterator end() const { return Iterator{ v_.end() }; }
            void push_back( std::shared_ptr<Layer> l ) { l->index = v_.size(); v_.push_back( std::move( l ) ); }
            const std::shared_ptr<Layer>& shared( size_t i ) const { return v_[ i ]; }
        private:
            Store v_;
        };

        GemmaTransformer( const GemmaConfig& cfg, dim_t max_seq, dim_t max_prefill, DeviceId device = Compute::Device::Rocm( 0 ) )
            : cfg_( cfg ), max_seq_( max_seq ), max_prefill_( std::max<dim_t>( max_prefill, 1 ) )
        {
            cfg_.validate();
            if ( cfg_.kv_fp8_rows ) cfg_.kv_fp8 = true;      // the rows switch implies the cache policy; at max_batch 1 this IS the kv_fp8 model
            if ( cfg_.bounded_local_kv_rows ) cfg_.bounded_local_kv = true;      // likewise: at max_batch 1 this IS the bounded_local_kv model
            if ( max_seq <= 0 ) throw std::invalid_argument( "GemmaTransformer: max_seq must be positive" );
            owned_ctx_ = Compute::createExecutionContext( device );
            ctx_ = Compute::cast_context<kDevice>( owned_ctx_.get() );
            buildAll();
        }

        ~GemmaTransformer()
        {
            destroyGraph();
            destroyGraphRows();
            destroyGraphChain();
            for ( auto& e : ov_ev_ ) if ( e ) (void)hipEventDestroy( e );
            if ( ov_stream_ ) (void)hipStreamDestroy( ov_stream_ );
        }

        Compute::RocmExecutionContext* context() const noexcept { return ctx_; }
        const GemmaConfig& config() const noexcept { return cfg_; }
        LayerList& layers() noexcept { return layers_; }

        // ------------------------------------------------------------------------------------
        // synthetic parameters: counter-based uniform values generated on the
        // device; Linear weights U(-1/sqrt(K), 1/sqrt(K)); norm weights 1 + 0.1 U(-1,1); table U(-a,a)
        // ------------------------------------------------------------------------------------
        /// multipliers on the generator above.  The defaults are SURVEY.md's unit-scale random weights, under which a bf16 rounding
        /// difference grows ~1.4x per block; a CONDITIONED profile (small post-norm weights = small residual updates, q/k norm weights
        /// that keep scores O(1), a layer scalar != 1, a larger embedding scale) behaves like a trained model: differences stay at the
        /// rounding floor, so whole-model logits can be held to 1e-3 (tests/test_gemma_conditioned_gpu.py, tests/ref_gemma.py)
        struct SyntheticProfile { float linear_gain = 1.0f, qk_norm_center = 1.0f, post_norm_center = 1.0f, layer_scalar = 1.0f, table_gain = 1.0f; };

        void initSynthetic( uint64_t seed, const SyntheticProfile& pr = SyntheticProfile{} )
        {
            destroyGraph();   // layer scalars are baked into the captured launches
            destroyGraphRows();
            destroyGraphChain();
            // the staging buffer holds the largest matrix of the model: the table, fc_gate_up, or -- on geometries whose attention is wider than the stream -- a packed qkv
            const dim_t attn_w = cfg_.num_heads * std::max( cfg_.head_dim, cfg_.global_head_dim );
            const dim_t qkv_w = attn_w + 2 * std::max( cfg_.num_kv_heads * cfg_.head_dim, cfg_.num_global_kv_heads * cfg_.global_head_dim );
            const size_t max_elems = static_cast<size_t>( std::max( { cfg_.vocab_size * cfg_.embedding_dim, cfg_.embedding_dim * 2 * cfg_.hidden_dim, cfg_.embedding_dim * qkv_w } ) );
            TensorType staging( ctx_->getDeviceId(), shape_t{ static_cast<dim_t>( max_elems ) } );
            auto fillLinear = [&]( auto& lin, uint64_t s, float gain )
            {
                const dim_t N = lin.getConfig().getOutputFeatures(), K = lin.getConfig().getInputFeatures();
                fill( staging.data(), N * K, s, gain / std::sqrt( static_cast<float>( K ) ), 0.0f );
                lin.loadWeightFromDevice( staging.data() );
                ctx_->synchronize();
            };
            auto fillNorm = [&]( RmsNormType& n, uint64_t s, float center = 1.0f ) { fill( n.getWeight()->data(), n.getConfig().dim(), s, 0.1f * center, center ); };
            for ( size_t i = 0; i < layers_.size(); ++i )
            {
                auto& L = layers_[ i ];
                const uint64_t b = seed * 1000003ull + i * 64ull;
                fillLinear( *L.qkv_proj, b + 1, pr.linear_gain ); fillLinear( *L.o_proj, b + 2, pr.linear_gain ); fillLinear( *L.fc_gate_up, b + 3, pr.linear_gain ); fillLinear( *L.fc_down, b + 4, pr.linear_gain );
                fillNorm( *L.input_norm, b + 5 ); fillNorm( *L.q_norm, b + 6, pr.qk_norm_center ); fillNorm( *L.k_norm, b + 7, pr.qk_norm_center );
                fill( L.v_norm->getWeight()->data(), L.v_norm->getConfig().dim(), 0, 0.0f, 1.0f );   // unit weight (Gemma.Block.ixx:880-886)
                fillNorm( *L.post_attn_norm, b + 8, pr.post_norm_center ); fillNorm( *L.pre_ffn_norm, b + 9 ); fillNorm( *L.post_ffn_norm, b + 10, pr.post_norm_center );
                L.layer_scalar = pr.layer_scalar;
            }
            fillNorm( *final_norm_, seed * 1000003ull + 64ull * layers_.size() + 1 );
            fillLinear( *lm_head_, seed * 1000003ull + 64ull * layers_.size() + 2, pr.table_gain );   // the tied table
            ctx_->synchronize();
        }

        // ------------------------------------------------------------------------------------
        // reference-order decode: one component forward per line of GemmaBlock::decode
        // ------------------------------------------------------------------------------------
        LogitsTensor& decode( const TokenTensor& token, dim_t position )
        {
            Compute::TraceRange tr( "gemma.decode(reference order)" );
            checkPosition( position, 1 );
            kv_fill_ = position + 1;
            embed( token.data(), 1, *hidden_[ 0 ] );
            TensorType* x = hidden_[ 0 ].get();
            for ( auto& L : layers_ ) x = &L.decode( x->view( shape_t{ 1, 1, cfg_.embedding_dim } ), position );
            auto& normed = final_norm_->forward( x->view( shape_t{ 1, 1, cfg_.embedding_dim } ) );
            head( normed.data() );
            return *logits_;
        }

        // ------------------------------------------------------------------------------------
        // fused decode: embedding + 6 launches per layer (7 over the FP8 KV cache) + head
        // ------------------------------------------------------------------------------------
        LogitsTensor& decodeFused( const TokenTensor& token, dim_t position )
        {
            Compute::TraceRange tr( "gemma.decode(fused)" );
            checkPosition( position, 1 );
            kv_fill_ = position + 1;
            enqueueFusedStep( token.data(), static_cast<int>( position ), nullptr );
            return *logits_;
        }

        /// SamplingParams (Components/Transformers/SamplingParams.ixx): temperature <= 0 is greedy; top_k 0 / top_p >= 1 disable
        /// the truncations.  The uniform r in [0, 1) is drawn by the caller, as in the reference (host RNG, GemmaModel.ixx:568).
        /// The four sampling filters (min_p, repetition / presence / frequency penalty; Operations.h, mila_cdna4.h: sampling filters) ride in the same struct, neutral
        /// by default.  The stochastic samplers take them from the SamplingParams they are given; the greedy samplers, which take none, from setSamplingFilters().
        /// The penalties depend on the tokens sampled so far, so their state -- one token table per row -- lives on the device and is updated by every filtered
        /// sampler, eager or captured: resetTokenTable() starts a request.  Log-probabilities are unchanged by all four: the samplers write their scaled copy into
        /// their own workspace and never touch the logits, so setStepLogprobs() keeps reporting the softmax of the soft-capped, UNPENALIZED logits.
        using SamplingParams = Compute::SamplingParams;

        /// the filters of the greedy samplers (sampleGreedy, sampleRowGreedy, the greedy captured steps); only the four filter fields of `f` are read.  With a penalty
        /// set, a greedy token is argmax of the adjusted logits (softcap first), ties to the lower id: the captured greedy step then ends at the logits, like the
        /// stochastic one, and runs the penalized sampler's two launches behind them.  min_p alone leaves a greedy request on today's path.  A change re-captures
        /// once, as a change of temperature does.  The token tables are allocated by the first call that sets a penalty, and counted in the memory statistics from
        /// then on; a model that never saw a penalty allocates nothing.
        void setSamplingFilters( const SamplingParams& f )
        {
            f.checkFilters( "GemmaTransformer::setSamplingFilters" );
            if ( f.penalized() ) ensureTokenTable();
            filters_ = onlyFilters( f );
        }
        const SamplingParams& samplingFilters() const noexcept { return filters_; }
        /// a new request on row `row` (0 for the one-sequence interface): every count to zero, the flag of each of the n prompt tokens set -- the WHOLE prompt, a
        /// KV-reused prefix included.  Stream-ordered; the ids are consumed before the call returns.
        void resetTokenTable( int row, const int32_t* prompt_host, size_t n )
        {
            ensureTokenTable();
            token_table_->reset( row, prompt_host, n );
            ctx_->synchronize();
        }
        /// the tables (nullptr before the first penalty or resetTokenTable())
        Compute::RocmTokenTable* tokenTable() noexcept { return token_table_.get(); }

        /// Logit bias (mila_cdna4.h: logit bias; Mila/TokenBias.h composes a request's logit_bias / banned / allowed / min_tokens into one): a table of vocab fp32
        /// values, finite or -inf, added to the capped logit ahead of the penalties by every sampler of this network but the chain step's -- the eager samplers, the
        /// one-row captured step and the rows step (one table for every row), greedy and stochastic.  setTokenBias() writes the whole table (every value `fill`, then
        /// values[j] at ids[j]) and turns the bias on; updateTokenBias() changes entries of a table that is on; clearTokenBias() turns it off.  Whether a bias is on
        /// belongs to what each graph was captured for, as the filters do: turning it on or off re-captures once; changing the table's contents never does, because
        /// the table's address is what is captured.  With a bias a greedy token is argmax of the adjusted logits: the greedy steps then end at the logits and run the
        /// penalized greedy sampler's two launches.  Log-probabilities stay those of the unbiased logits.  The table is allocated by the first setTokenBias() and
        /// counted in the memory statistics from then on.  The caller keeps at least one token finite.
        void setTokenBias( float fill, const int32_t* ids_host, const float* values_host, size_t n )
        {
            if ( std::isnan( fill ) || ( std::isinf( fill ) && fill > 0.0f ) ) throw std::invalid_argument( "GemmaTransformer::setTokenBias: the fill value must be finite or -inf" );
            checkBiasEntries( ids_host, values_host, n, "GemmaTransformer::setTokenBias" );
            if ( !token_bias_ ) token_bias_ = std::make_unique<Compute::RocmTokenBias>( ctx_, cfg_.vocab_size );
            token_bias_->apply( fill, ids_host, values_host, n );
            bias_on_ = true;
            if ( automaton_on_ ) token_automaton_->compose( biasValues() );      // the effective table follows its base
        }
        void updateTokenBias( const int32_t* ids_host, const float* values_host, size_t n )
        {
            if ( !bias_on_ ) throw std::logic_error( "GemmaTransformer::updateTokenBias: no bias is set (setTokenBias)" );
            checkBiasEntries( ids_host, values_host, n, "GemmaTransformer::updateTokenBias" );
            token_bias_->update( ids_host, values_host, n );
            if ( automaton_on_ ) token_automaton_->compose( biasValues() );
        }
        /// an update uploaded now and enqueued later: commitTokenBiasUpdate() is one small launch in stream order that reads no host memory -- what a decode-ahead
        /// loop puts between two replays (GemmaModel: the min_tokens restore)
        void stageTokenBiasUpdate( const int32_t* ids_host, const float* values_host, size_t n )
        {
            if ( !bias_on_ ) throw std::logic_error( "GemmaTransformer::stageTokenBiasUpdate: no bias is set (setTokenBias)" );
            checkBiasEntries( ids_host, values_host, n, "GemmaTransformer::stageTokenBiasUpdate" );
            token_bias_->stage( ids_host, values_host, n );
        }
        void commitTokenBiasUpdate()
        {
            if ( !bias_on_ ) throw std::logic_error( "GemmaTransformer::commitTokenBiasUpdate: no bias is set (setTokenBias)" );
            token_bias_->commit();
            if ( automaton_on_ ) token_automaton_->compose( biasValues() );
        }
        void clearTokenBias()
        {
            const bool was = bias_on_;
            bias_on_ = false;
            if ( was && automaton_on_ ) token_automaton_->compose( nullptr );
        }
        bool tokenBiasOn() const noexcept { return bias_on_; }
        /// the table (nullptr before the first setTokenBias())
        Compute::RocmTokenBias* tokenBias() noexcept { return token_bias_.get(); }

        /// Token automaton (mila_cdna4.h: token automaton; Mila/TokenAutomaton.h): grammar-constrained decoding on the one-row interface.  While one is on, every one-row
        /// sampler of this network -- sampleGreedy / sampleStochasticRadix and the tail of the captured step -- reads the automaton's effective table (the bias table, or
        /// zeros, with -inf wherever the current state forbids the token) in the place of the bias table and is followed by ONE launch that advances the state by the
        /// token just chosen and rewrites the table: a node behind the tail of a captured step, the same launch behind an eager sampler.  A greedy step then ends at
        /// the logits and takes the biased greedy sampler's two launches.  setTokenAutomaton() validates, uploads, turns it on and resets; resetTokenAutomaton() puts
        /// the state back to `start` and composes the table; clearTokenAutomaton() turns it off.  Whether one is on belongs to what the one-row graph was captured
        /// for, with the image's address and (S, C), which the step node holds by value: on / off re-captures once, as does an automaton of another size; replacing
        /// the contents of one of the same size, or resetting, never does.  The rows step and the chain step refuse while one is on.  Log-probabilities stay those
        /// of the unconstrained logits.  Allocated by the first setTokenAutomaton() and counted in the memory statistics from then on.
        void setTokenAutomaton( const TokenAutomaton& a )
        {
            a.validate( cfg_.vocab_size );
            if ( !token_automaton_ ) token_automaton_ = std::make_unique<Compute::RocmTokenAutomaton>( ctx_, cfg_.vocab_size, cfg_.draft_tokens );
            token_automaton_->upload( a.class_of.data(), a.next.data(), a.num_states, a.num_classes, a.start );
            automaton_on_ = true;
            token_automaton_->reset( biasValues() );
        }
        void resetTokenAutomaton()
        {
            if ( !automaton_on_ ) throw std::logic_error( "GemmaTransformer::resetTokenAutomaton: no automaton is set (setTokenAutomaton)" );
            token_automaton_->reset( biasValues() );
        }
        void clearTokenAutomaton() noexcept { automaton_on_ = false; }
        bool tokenAutomatonOn() const noexcept { return automaton_on_; }
        /// the state word, read synchronously: for tests, and for a caller that asks whether the final state is accepting
        int32_t tokenAutomatonState()
        {
            if ( !token_automaton_ || !token_automaton_->loaded() ) throw std::logic_error( "GemmaTransformer::tokenAutomatonState: no automaton was set (setTokenAutomaton)" );
            return token_automaton_->readState();
        }
        /// the device side (nullptr before the first setTokenAutomaton())
        Compute::RocmTokenAutomaton* tokenAutomaton() noexcept { return token_automaton_.get(); }

        /// capture the fused step once; afterwards replayGraph() advances one token per call.
        /// The token is read from `token` (device) and the position from an internal device counter.
        /// Every device pointer the captured nodes hold is model-owned and fixed for the model's lifetime (the split-attention partials
        /// live in attn_partials_, never in the growable context scratch), so a later prefill or Linear::forward that grows the context
        /// scratch cannot leave the graph pointing at freed memory.  A second capture replaces the first (the old graph is destroyed).
        void captureGraph( const TokenTensor& token, dim_t start_position )
        {
            Compute::TraceRange tr( "gemma.captureGraph" );
            setDevicePosition( start_position );
            destroyGraph();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx_->getStream() );
            ctx_->synchronize();
            hipCheck( hipStreamBeginCapture( s, hipStreamCaptureModeThreadLocal ), "hipStreamBeginCapture" );
            hipGraph_t g = nullptr;
            try
            {
                // greedy sampler (feeds the next replay) + position bump + publication of the token.  The sampler's FIRST stage runs in the lm_head's epilogue (every
                // workgroup leaves its best logit and index in the sampler scratch), its final reduction does the other three: one launch behind the head, not three
                int sampler_partials = 0;
                captured_band_end_ = bandBucket( start_position );
                const bool stochastic = graph_sampling_.has_value();
                const bool penalized_greedy = sample_in_graph_ && !stochastic && ( filters_.penalized() || bias_on_ || automaton_on_ );      // ends at the logits; the penalized sampler's two launches follow
                if ( stochastic && ( !draw_ring_ || !token_seq_ ) )
                    throw std::invalid_argument( "GemmaTransformer::captureGraph: a stochastic step needs setDrawRing() and the sequence counter of setTokenRing()" );
                if ( step_lp_ && !stochastic && !sample_in_graph_ )
                    throw std::invalid_argument( "GemmaTransformer::captureGraph: token log-probabilities need a sampler in the step (setSampleInGraph / setGraphSampling)" );
                enqueueFusedStep( token.data(), static_cast<int>( captured_band_end_ ), pos_dev_->data(), ( sample_in_graph_ && !stochastic && !penalized_greedy ) ? &sampler_partials : nullptr );
                // stochastic: the step ends at the logits like the sampler-less one, then the radix pipeline on the model-owned workspace; its last node draws from the
                // ring, writes the next token, bumps the position and publishes -- in the place of the advance_position node.  One linear chain on one stream.
                if ( stochastic && ( graph_sampling_->filtered() || bias_on_ || automaton_on_ ) )      // the same launches, in their filtered / biased instantiations: the node count does not move
                {
                    const mila_sample_filters f = graph_sampling_->filters();
                    Compute::rocmCheck( mila_cdna4_sample_radix_biased_advance_fp32( logits_->data(), const_cast<TokenTensor&>( token ).data(), (int)cfg_.vocab_size,
                                                                                     cfg_.final_logit_softcapping, graph_sampling_->temperature, graph_sampling_->top_k,
                                                                                     graph_sampling_->top_p, draw_ring_, draw_ring_size_, &f, tableWords( *graph_sampling_, 0, false ),
                                                                                     samplerBias(), 0, radix_scratch_->data(), radix_scratch_->sizeInBytes(), pos_dev_->data(), token_seq_,
                                                                                     token_ring_, token_ring_ ? token_ring_size_ : 0, ctx_->getStream() ) );
                }
                else if ( stochastic )
                    Compute::rocmCheck( mila_cdna4_sample_radix_advance_fp32( logits_->data(), const_cast<TokenTensor&>( token ).data(), (int)cfg_.vocab_size, cfg_.final_logit_softcapping,
                                                                              graph_sampling_->temperature, graph_sampling_->top_k, graph_sampling_->top_p, draw_ring_, draw_ring_size_,
                                                                              radix_scratch_->data(), radix_scratch_->sizeInBytes(), pos_dev_->data(), token_seq_, token_ring_,
                                                                              token_ring_ ? token_ring_size_ : 0, ctx_->getStream() ) );
                else if ( penalized_greedy )
                {
                    const mila_sample_filters f = filters_.filters();
                    Compute::rocmCheck( mila_cdna4_sample_argmax_biased_advance_fp32( logits_->data(), const_cast<TokenTensor&>( token ).data(), (int)cfg_.vocab_size,
                                                                                      cfg_.final_logit_softcapping, &f, tableWords( filters_, 0, false ), samplerBias(), 0,
                                                                                      sample_scratch_->data(), sample_scratch_->sizeInBytes(), pos_dev_->data(),
                                                                                      token_ring_ ? token_seq_ : nullptr, token_ring_, token_ring_ ? token_ring_size_ : 0, ctx_->getStream() ) );
                }
                else if ( sample_in_graph_ )
                    Compute::rocmCheck( mila_cdna4_sample_argmax_final_advance( const_cast<TokenTensor&>( token ).data(), sample_scratch_->data(), sample_scratch_->sizeInBytes(), sampler_partials,
                                                                                pos_dev_->data(), token_ring_ ? token_seq_ : nullptr, token_ring_, token_ring_ ? token_ring_size_ : 0,
                                                                                ctx_->getStream() ) );
                else
                    Compute::rocmCheck( mila_cdna4_advance_position( pos_dev_->data(), ctx_->getStream() ) );
                // a token automaton: one more node behind the tail, which reads the token word the tail wrote, advances the state and rewrites the effective table the
                // next replay's sampler reads
                if ( automaton_on_ && ( sample_in_graph_ || stochastic ) ) token_automaton_->step( biasValues(), token.data() );
                // the tail has written the next token (and bumped the sequence counter): its log-probability and the alternatives, two more nodes
                if ( step_lp_ ) enqueueStepLogprobs( token.data() );
            }
            catch ( ... ) { (void)hipStreamEndCapture( s, &g ); if ( g ) (void)hipGraphDestroy( g ); throw; }
            hipCheck( hipStreamEndCapture( s, &g ), "hipStreamEndCapture" );
            graph_ = g;
            const hipError_t e = hipGraphInstantiate( &graph_exec_, graph_, nullptr, nullptr, 0 );
            if ( e != hipSuccess ) { graph_exec_ = nullptr; destroyGraph(); hipCheck( e, "hipGraphInstantiate" ); }
            captured_token_ = token.data();
            captured_sample_in_graph_ = sample_in_graph_;
            captured_ring_ = token_ring_;
            captured_sampling_ = graph_sampling_;
            captured_filters_ = filters_;
            captured_bias_ = bias_on_;
            captured_automaton_ = automatonKey();
            captured_draw_ring_ = graph_sampling_ ? draw_ring_ : nullptr;
            captured_lp_ = step_lp_;
            ++graph_captures_;
        }
        /// capture on first use, and again whenever the captured graph no longer matches what a replay must do: another token
        /// buffer, or a different sampler setting (a graph captured without the sampler node never writes the next token)
        /// ... or a position in another band bucket than the attention launches were captured for (an unwindowed layer's split geometry and kernel form follow the live-length
        /// bucket -- 4096, 8192, 16384, ... keys, clipped to the capacity -- not the cache capacity).  Cheap: callers invoke it before every replay.
        void ensureGraph( const TokenTensor& token, dim_t start_position )
        {
            if ( !graph_exec_ || captured_token_ != token.data() || captured_sample_in_graph_ != sample_in_graph_ || captured_ring_ != token_ring_ ||
                 !sameSampling( captured_sampling_, graph_sampling_ ) || ( graph_sampling_ && captured_draw_ring_ != draw_ring_ ) || captured_lp_ != step_lp_ ||
                 ( sample_in_graph_ && !graph_sampling_ && !samePenalties( captured_filters_, filters_ ) ) ||
                 ( ( sample_in_graph_ || graph_sampling_ ) && captured_bias_ != bias_on_ ) ||
                 ( ( sample_in_graph_ || graph_sampling_ ) && captured_automaton_ != automatonKey() ) ||
                 bandBucket( start_position ) != captured_band_end_ )
                captureGraph( token, start_position );
        }
        /// the live-length bucket of a position, asked of the device library whose launches follow it
        dim_t bandBucket( dim_t position ) const
        {
            return mila_cdna4_attn_decode_band_bucket( static_cast<int>( position + 1 ), static_cast<int>( max_seq_ ) );
        }
        bool graphCaptured() const noexcept { return graph_exec_ != nullptr; }
        /// kernel nodes of the captured decode step (0 before a capture): the launches one token costs on the graph path
        size_t graphNodeCount() const
        {
            if ( !graph_ ) return 0;
            size_t n = 0;
            hipCheck( hipGraphGetNodes( graph_, nullptr, &n ), "hipGraphGetNodes" );
            return n;
        }
        /// captures so far: the first use, and one more for every change ensureGraph() answered (another token buffer, sampler setting, ring, or band bucket)
        size_t graphCaptureCount() const noexcept { return graph_captures_; }
        bool graphSamples() const noexcept { return graph_exec_ != nullptr && captured_sample_in_graph_; }
        /// when set, every replay ends with the greedy sampler writing the next token into the token buffer the graph reads from:
        /// a closed autoregressive loop with no host round trip.  Takes effect at the next ensureGraph() / captureGraph().
        void setSampleInGraph( bool on ) { sample_in_graph_ = on; }
        /// a caller-owned token ring in host-visible memory + its device sequence counter (GemmaModel's decode-ahead loop): with the sampler in the graph, the
        /// step's last node publishes the sampled token there (mila_cdna4_advance_position_snapshot).  Takes effect at the next ensureGraph(); nullptr = off
        void setTokenRing( unsigned long long* ring, int size, unsigned long long* seq_dev )
        {
            if ( ring && ( size <= 0 || !seq_dev ) ) throw std::invalid_argument( "GemmaTransformer::setTokenRing: a ring needs a positive size and a sequence counter" );
            token_ring_ = ring; token_ring_size_ = ring ? size : 0; token_seq_ = ring ? seq_dev : nullptr;
        }
        /// the stochastic sampler as the tail of the captured step (the radix pipeline, mila_cdna4_sample_radix_advance_fp32): with `sp` set, a capture ends at the
        /// logits and runs the sampler's launches behind them, the last of which takes the place of the position bump; nullopt = off (the greedy / sampler-less
        /// capture that setSampleInGraph() chooses).  Needs setDrawRing() and setTokenRing()'s sequence counter.  ensureGraph() re-captures when temperature, top_k or
        /// top_p differ from what was captured.  sp.temperature must be > 0.
        void setGraphSampling( const std::optional<SamplingParams>& sp )
        {
            if ( sp && !( sp->temperature > 0.0f ) ) throw std::invalid_argument( "GemmaTransformer::setGraphSampling: temperature must be > 0 (greedy: setSampleInGraph)" );
            if ( sp ) sp->checkFilters( "GemmaTransformer::setGraphSampling" );
            if ( sp && sp->penalized() ) ensureTokenTable();      // (never inside a capture)
            graph_sampling_ = sp;
        }
        /// the uniform draws of the captured stochastic step: `size` floats of host-visible memory (device address); sample number n (the sequence counter's value after
        /// it) reads slot n % size, which the host fills before it launches the replay that consumes it
        void setDrawRing( const float* draws, int size )
        {
            if ( draws && size <= 0 ) throw std::invalid_argument( "GemmaTransformer::setDrawRing: a ring needs a positive size" );
            draw_ring_ = draws; draw_ring_size_ = draws ? size : 0;
        }
        /// token log-probabilities as part of every step (mila_cdna4_token_logprobs_*): with top_n set (0 .. 20; 0 = the chosen token's only), the one-row step, the
        /// rows step and the chain step run the two log-probability launches behind their sampler tail -- the tail decides the token, and a captured step is one
        /// linear chain, so nothing is gained by placing the partials launch earlier.  The one-row step publishes a record into `ring` (device address of ring_size
        /// records of RocmTokenLogprobsOp::recordWords() host-visible 32-bit words, slot = the sequence counter of setTokenRing(), which the tail has already bumped)
        /// or, without a ring, writes the op's device outputs; the rows step reports the active rows, the chain step the accepted ones, both into the device outputs
        /// (tokenLogprobs().read()).  A step without a sampler tail has no token to report: capturing or running one with the setting on is an invalid_argument.
        /// The scratch and the outputs are allocated by the first call that turns the setting on, and counted in the memory statistics from then on; with the
        /// setting off a step is launch for launch what it is without this interface.  ensureGraph*() re-capture when the setting changes.
        void setStepLogprobs( std::optional<int> top_n, uint32_t* ring = nullptr, int ring_size = 0 )
        {
            if ( !top_n ) { step_lp_.reset(); return; }
            if ( ring ? ring_size <= 0 : ring_size != 0 ) throw std::invalid_argument( "GemmaTransformer::setStepLogprobs: a ring and a positive ring size go together" );
            if ( *top_n < 0 || *top_n > std::min<dim_t>( Compute::RocmTokenLogprobsOp::kMaxTop, cfg_.vocab_size ) )
                throw std::invalid_argument( "GemmaTransformer::setStepLogprobs: top_n " + std::to_string( *top_n ) + " outside 0 .. min(20, vocabulary)" );
            if ( !lp_op_ )
                lp_op_ = std::make_unique<Compute::RocmTokenLogprobsOp>( ctx_, Compute::TokenLogprobsOpConfig{ cfg_.vocab_size, cfg_.final_logit_softcapping,
                                                                                                                   static_cast<int>( rows_ ? rowsCount() : 1 ) } );
            step_lp_ = StepLogprobs{ *top_n, ring, ring_size };
        }
        std::optional<int> stepLogprobs() const noexcept { return step_lp_ ? std::optional<int>( step_lp_->top_n ) : std::nullopt; }
        /// the op behind setStepLogprobs() (its device outputs); only after the setting was turned on once
        Compute::RocmTokenLogprobsOp& tokenLogprobs()
        {
            if ( !lp_op_ ) throw std::logic_error( "GemmaTransformer::tokenLogprobs: setStepLogprobs() first" );
            return *lp_op_;
        }
        /// the one-row step's two launches for an EAGER step: `token_dev` holds the token a sampler just chose from logits() (and, in the ring form, snapshot_token or
        /// the tail has bumped the sequence counter for it).  A captured one-row step runs them itself.
        void enqueueStepLogprobs( const int32_t* token_dev )
        {
            if ( !step_lp_ ) throw std::logic_error( "GemmaTransformer::enqueueStepLogprobs: setStepLogprobs() first" );
            if ( step_lp_->ring )
            {
                if ( !token_seq_ ) throw std::invalid_argument( "GemmaTransformer: the log-probability ring needs the sequence counter of setTokenRing()" );
                lp_op_->publish( logits_->data(), token_dev, step_lp_->top_n, token_seq_, step_lp_->ring, step_lp_->ring_size );
            }
            else
                lp_op_->forward( logits_->data(), static_cast<size_t>( cfg_.vocab_size ), token_dev, 1, step_lp_->top_n, nullptr, nullptr );
        }
        /// the same for row b of the rows interface alone, behind sampleRowGreedy / sampleRowStochastic (a row's first token, from its prefill's logits): the
        /// outputs land in row 0 of the op's
        void enqueueRowLogprobs( int b )
        {
            requireRows( b );
            if ( !step_lp_ ) throw std::logic_error( "GemmaTransformer::enqueueRowLogprobs: setStepLogprobs() first" );
            lp_op_->forward( rows_->logits->data() + static_cast<size_t>( b ) * cfg_.vocab_size, static_cast<size_t>( cfg_.vocab_size ), rows_->tok->data() + b, 1, step_lp_->top_n,
                             nullptr, nullptr );
        }
        bool sampleInGraph() const noexcept { return sample_in_graph_; }
        void setDevicePosition( dim_t position )
        {
            checkPosition( position, 1 );
            const int32_t p = static_cast<int32_t>( position );
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( pos_dev_->data(), &p, 4, ctx_->getStream() ) );
            ctx_->synchronize();
        }
        void replayGraph()
        {
            if ( !graph_exec_ ) throw std::runtime_error( "GemmaTransformer::replayGraph: captureGraph() first" );
            Compute::TraceRange tr( "gemma.decode(graph replay)" );
            hipCheck( hipGraphLaunch( graph_exec_, reinterpret_cast<hipStream_t>( ctx_->getStream() ) ), "hipGraphLaunch" );
        }
        LogitsTensor& logits() { return *logits_; }

        // ------------------------------------------------------------------------------------
        // batched decode (GemmaConfig::max_batch > 1): up to four INDEPENDENT sequences per step, row b at its own position rows_->pos[ b ], on its own KV caches.
        // A step is enqueueFusedStep's launch sequence on the rows entries (matvec_rows, fused_attn_decode_rows_bf16): six launches per layer, the weights streamed
        // once for all rows, always in the device-position form.  Row b's logits are bit-identical to the same sequence run alone through decodeFused(), as long as
        // both runs are in the same live-length bucket (mila_cdna4.h: fused_attn_decode_rows_bf16).  With GemmaConfig::kv_fp8_rows every row has its own FP8 KV
        // caches and the attention launch is two -- fused_qkv_post_kvfp8_rows_devpos into the rows q buffer, attn_decode_kvfp8_rows -- seven per layer, one linear
        // chain; row b is then bit-identical to the same sequence alone on a kv_fp8 model.  prefillRow / forkRow / forkRowPrefix / rewindKvCacheRow / resetRow work on
        // either cache: a row's state beside its caches is its position word, its token and its logits.
        // ------------------------------------------------------------------------------------
        dim_t maxBatch() const noexcept { return cfg_.max_batch; }
        /// the capacity of the sliding-window layers' rings on a rows model built with GemmaConfig::bounded_local_kv_rows (0: every row on flat caches) -- with
        /// config().window the geometry PrefixCache takes
        dim_t rowsRingCapacity() const noexcept { return ring_capacity_; }
        /// prefill `n` tokens at positions offset .. into row b's caches through the B = 1 prefill (cache-row selection; no prefill kernel knows about rows); row b's
        /// logits and position word follow.  The row's first decode token is the caller's to set (setRowToken).
        LogitsTensor& prefillRow( int b, const TokenTensor& tokens, dim_t n, dim_t offset = 0 )
        {
            requireRows( b );
            if ( n <= 0 ) throw std::invalid_argument( "GemmaTransformer::prefillRow: empty prompt" );
            if ( ringRows() )      // (before the first chunk writes: a prefill that throws half way has still written)
            {
                if ( offset == 0 ) row_high_[ static_cast<size_t>( b ) ] = row_from_[ static_cast<size_t>( b ) ] = 0;
                else if ( !rowHolds( b, offset ) )
                    throw std::invalid_argument( "GemmaTransformer::prefillRow: row " + std::to_string( b ) + "'s rings no longer hold what a continuation from " + std::to_string( offset ) +
                                                 " reads (valid from " + std::to_string( rowValidFrom( b ) ) + ", window " + std::to_string( cfg_.window ) + ")" );
                row_high_[ static_cast<size_t>( b ) ] = std::max( row_high_[ static_cast<size_t>( b ) ], offset + n );
            }
            for ( auto& L : layers_ ) L.selectCacheRow( b );
            try
            {
                for ( dim_t p0 = 0; p0 < n; p0 += max_prefill_ )      // chunks of the built prefill size, as prefillFrom() does
                {
                    const dim_t c = std::min( max_prefill_, n - p0 );
                    prefill( tokens.slice( static_cast<size_t>( p0 ), shape_t{ 1, c } ), c, offset + p0 );
                }
            }
            catch ( ... ) { for ( auto& L : layers_ ) L.selectCacheRow( 0 ); throw; }
            for ( auto& L : layers_ ) L.selectCacheRow( 0 );
            Compute::rocmCheck( mila_cdna4_memcpy_d2d( rows_->logits->data() + static_cast<size_t>( b ) * cfg_.vocab_size, logits_->data(), static_cast<size_t>( cfg_.vocab_size ) * 4, ctx_->getStream() ) );
            setRowWord( rows_->pos->data(), b, static_cast<int32_t>( offset + n ) );
            return *logits_;
        }
        /// forget row b: position 0, inactive (its caches are overwritten positionally by the next prefillRow)
        void resetRow( int b ) { requireRows( b ); setRowWord( rows_->pos->data(), b, 0 ); setRowWord( rows_->active->data(), b, 0 ); noteRowActive( b, false ); }
        /// rewindKvCache for one row: row b goes on from `position`, given that `written` positions were appended to it; its caches are overwritten positionally.
        /// false when the request is out of range; on a ring model (bounded_local_kv_rows) also by the ring rule of RocmGqaOpBase::rewindKvCache, per row: when
        /// written - position > capacity - window, or when the row's valid-from bound (a band fork's, or the furthest the row was ever written less the capacity) lies
        /// above position - window.  A refused row is prefilled from 0, which overwrites positionally.
        bool rewindKvCacheRow( int b, dim_t position, dim_t written )
        {
            requireRows( b );
            if ( position < 0 || position > written || written > max_seq_ ) return false;
            if ( ringRows() )
            {
                row_high_[ static_cast<size_t>( b ) ] = std::max( row_high_[ static_cast<size_t>( b ) ], written );
                if ( written - position > ring_capacity_ - cfg_.window || !rowHolds( b, position ) ) return false;
            }
            setRowWord( rows_->pos->data(), b, static_cast<int32_t>( position ) );
            return true;
        }
        void setRowActive( int b, bool on ) { requireRows( b ); setRowWord( rows_->active->data(), b, on ? 1 : 0 ); noteRowActive( b, on ); }
        void setRowToken( int b, int32_t token ) { requireRows( b ); setRowWord( rows_->tok->data(), b, token ); }
        void setRowPosition( int b, dim_t position ) { requireRows( b ); checkPosition( position, 1 ); setRowWord( rows_->pos->data(), b, static_cast<int32_t>( position ) ); }
        /// row b's next token from row b's logits, into the rows token buffer: the greedy sampler, or the radix pipeline at the caller's draw r (the sampler
        /// generate() uses, on the model-owned one-row workspaces)
        void sampleRowGreedy( int b ) { sampleRowGreedyWith( b, filters_ ); }
        void sampleRowGreedyWith( int b, const SamplingParams& fl )
        {
            requireRows( b );
            if ( fl.penalized() || bias_on_ )
            {
                const mila_sample_filters f = fl.filters();
                Compute::rocmCheck( mila_cdna4_sample_argmax_biased_fp32( rows_->logits->data() + static_cast<size_t>( b ) * cfg_.vocab_size, rows_->tok->data() + b, (int)cfg_.vocab_size,
                                                                          cfg_.final_logit_softcapping, &f, tableWords( fl, b, true ), biasValues(), 0, sample_scratch_->data(),
                                                                          sample_scratch_->sizeInBytes(), ctx_->getStream() ) );
                return;
            }
            Compute::rocmCheck( mila_cdna4_sample_argmax_fp32( rows_->logits->data() + static_cast<size_t>( b ) * cfg_.vocab_size, rows_->tok->data() + b, (int)cfg_.vocab_size,
                                                               sample_scratch_->data(), sample_scratch_->sizeInBytes(), ctx_->getStream() ) );
        }
        void sampleRowStochastic( int b, const SamplingParams& sp, float r )
        {
            if ( sp.temperature <= 0.0f ) { sampleRowGreedyWith( b, sp.filtered() ? sp : filters_ ); return; }
            requireRows( b );
            if ( sp.filtered() || bias_on_ )
            {
                sp.checkFilters( "GemmaTransformer::sampleRowStochastic" );
                const mila_sample_filters f = sp.filters();
                Compute::rocmCheck( mila_cdna4_sample_radix_biased_fp32( rows_->logits->data() + static_cast<size_t>( b ) * cfg_.vocab_size, rows_->tok->data() + b, (int)cfg_.vocab_size,
                                                                         cfg_.final_logit_softcapping, sp.temperature, sp.top_k, sp.top_p, r, &f, tableWords( sp, b, true ), biasValues(), 0,
                                                                         radix_scratch_->data(), radix_scratch_->sizeInBytes(), ctx_->getStream() ) );
                return;
            }
            Compute::rocmCheck( mila_cdna4_sample_radix_fp32( rows_->logits->data() + static_cast<size_t>( b ) * cfg_.vocab_size, rows_->tok->data() + b, (int)cfg_.vocab_size,
                                                              cfg_.final_logit_softcapping, sp.temperature, sp.top_k, sp.top_p, r, radix_scratch_->data(), radix_scratch_->sizeInBytes(),
                                                              ctx_->getStream() ) );
        }
        LogitsTensor& rowsLogits() { requireRows( 0 ); return *rows_->logits; }
        TokenTensor& rowsTokens() { requireRows( 0 ); return *rows_->tok; }
        TokenTensor& rowsPositions() { requireRows( 0 ); return *rows_->pos; }

        /// one eager step over rows 0 .. B - 1 (2 <= B <= max_batch): the launches a captured rows step holds.  max_position: the largest position among the active
        /// rows (its live-length bucket shapes the attention launches).  greedy: the step ends with the rows sampler tail (next token and position bump of every
        /// active row); otherwise it ends at the logits and the position bump alone.
        void decodeRows( int B, dim_t max_position, bool greedy )
        {
            checkRowsStep( B, max_position );
            enqueueRowsStepAndTail( B, bandBucket( max_position ), greedy );
        }
        void captureGraphRows( int B, dim_t max_position, bool greedy )
        {
            checkRowsStep( B, max_position );
            Compute::TraceRange tr( "gemma.captureGraphRows" );
            destroyGraphRows();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx_->getStream() );
            ctx_->synchronize();
            hipCheck( hipStreamBeginCapture( s, hipStreamCaptureModeThreadLocal ), "hipStreamBeginCapture" );
            hipGraph_t g = nullptr;
            const dim_t band = bandBucket( max_position );
            try { enqueueRowsStepAndTail( B, band, greedy ); }      // one linear chain on one stream, like the one-row graph
            catch ( ... ) { (void)hipStreamEndCapture( s, &g ); if ( g ) (void)hipGraphDestroy( g ); throw; }
            hipCheck( hipStreamEndCapture( s, &g ), "hipStreamEndCapture" );
            rows_graph_ = g;
            const hipError_t e = hipGraphInstantiate( &rows_graph_exec_, rows_graph_, nullptr, nullptr, 0 );
            if ( e != hipSuccess ) { rows_graph_exec_ = nullptr; destroyGraphRows(); hipCheck( e, "hipGraphInstantiate" ); }
            rows_captured_B_ = B; rows_captured_greedy_ = greedy; rows_captured_band_ = band;
            rows_captured_sampling_ = rows_sampling_; rows_captured_draws_ = row_requests_.empty() ? rows_draws_ : row_request_draws_;
            rows_captured_filters_ = filters_;
            rows_captured_bias_ = bias_on_;
            rows_captured_lp_ = step_lp_;
            rows_captured_key_ = rowsRequestKey();
            ++rows_graph_captures_;
        }
        /// capture on first use and whenever the step changes: another row count, sampler tail, or the live-length bucket of the largest active row
        void ensureGraphRows( int B, dim_t max_position, bool greedy )
        {
            if ( !row_requests_.empty() )      // row requests: the class facts, the row count, the bucket and the log-probability setting -- no parameter of any row
            {
                if ( !rows_graph_exec_ || rows_captured_B_ != B || rows_captured_band_ != bandBucket( max_position ) || rows_captured_lp_ != step_lp_ || rows_captured_key_ != rowsRequestKey() ||
                     rows_captured_draws_ != row_request_draws_ )
                    captureGraphRows( B, max_position, greedy );
                return;
            }
            if ( !rows_graph_exec_ || rows_captured_key_.on || rows_captured_B_ != B || rows_captured_greedy_ != greedy || rows_captured_band_ != bandBucket( max_position ) || rows_captured_lp_ != step_lp_ ||
                 ( !greedy && ( !sameSampling( rows_captured_sampling_, rows_sampling_ ) || rows_captured_draws_ != rows_draws_ ) ) ||
                 ( greedy && !samePenalties( rows_captured_filters_, filters_ ) ) || ( ( greedy || rowsSamplesInStep() ) && rows_captured_bias_ != bias_on_ ) )
                captureGraphRows( B, max_position, greedy );
        }
        /// the stochastic sampler as the tail of a non-greedy rows step (mila_cdna4_sample_radix_rows_advance_fp32): with `sp` and `draws` set, decodeRows /
        /// captureGraphRows with greedy == false run the radix pipeline over the B rows behind the logits, and its tail -- token and position bump of every active
        /// row -- takes the place of advance_positions_rows.  draws: device address of max_batch floats of host-visible memory, row b's draw at [ b ], which the
        /// host writes before each step.  Both optional: nullopt / nullptr = the step ends at the logits and the position bump, as before.  ensureGraphRows()
        /// re-captures when either changes.
        void setRowsSampling( const std::optional<SamplingParams>& sp, const float* draws )
        {
            requireRows( 0 );
            if ( sp && !( sp->temperature > 0.0f ) ) throw std::invalid_argument( "GemmaTransformer::setRowsSampling: temperature must be > 0 (greedy: the greedy rows step)" );
            if ( sp ) sp->checkFilters( "GemmaTransformer::setRowsSampling" );
            if ( sp && sp->penalized() ) ensureTokenTable();
            rows_sampling_ = sp; rows_draws_ = draws;
        }
        /// ROW REQUESTS (mila_cdna4.h: row requests): rows 0 .. n - 1 of the rows step each sample under their OWN parameters -- temperature <= 0 makes a row greedy --
        /// from records in device memory, written here in stream order.  While requests are installed decodeRows / captureGraphRows / ensureGraphRows ignore their
        /// `greedy` argument and setRowsSampling's setting: the step ends in the requests tails (enqueueRowsRequestsStepAndTail).  draws: device address of max_batch
        /// floats of host-visible memory, row b's draw at [ b ] (needed when a row is stochastic).  The rows graph is captured again only when a CLASS fact changes
        /// (whether there are greedy rows, stochastic rows, a constrained row, a row with an automaton, a penalized row), never for other parameters of the same class.
        /// Every record is validated before anything is written.  clearRowsRequests() returns the rows step to the shared parameters.
        void setRowsRequests( std::span<const SamplingParams> requests, const float* draws )
        {
            requireRows( 0 );
            if ( requests.empty() || static_cast<dim_t>( requests.size() ) > cfg_.max_batch )
                throw std::invalid_argument( "GemmaTransformer::setRowsRequests: " + std::to_string( requests.size() ) + " requests for max_batch " + std::to_string( cfg_.max_batch ) );
            bool penalized = false;
            for ( size_t b = 0; b < requests.size(); ++b )
            {
                const auto& q = requests[ b ];
                const std::string who = "GemmaTransformer::setRowsRequests: row " + std::to_string( b );
                if ( !std::isfinite( q.temperature ) ) throw std::invalid_argument( who + ": temperature is not finite" );
                if ( q.top_k < 0 || !( q.top_p > 0.0f ) ) throw std::invalid_argument( who + ": need top_k >= 0, top_p > 0" );
                q.checkFilters( who.c_str() );
                penalized = penalized || q.penalized();
            }
            if ( penalized ) ensureTokenTable();
            if ( !row_params_ )
            {
                row_params_ = std::make_unique<TokenTensor>( ctx_->getDeviceId(), shape_t{ static_cast<dim_t>( mila_cdna4_sample_row_params_bytes( static_cast<int>( cfg_.max_batch ) ) / 4 ) } );
                Compute::rocmCheck( mila_cdna4_memset_zero( row_params_->rawData(), row_params_->sizeInBytes(), ctx_->getStream() ) );
            }
            for ( int b = 0; b < static_cast<int>( cfg_.max_batch ); ++b )      // a row without a request: greedy and neutral (it stays inactive)
            {
                const SamplingParams q = static_cast<size_t>( b ) < requests.size() ? requests[ static_cast<size_t>( b ) ] : SamplingParams{};
                mila_sample_row_params rec{};
                rec.temperature = static_cast<size_t>( b ) < requests.size() ? q.temperature : 0.0f;
                rec.top_k = q.top_k; rec.top_p = q.top_p; rec.min_p = q.min_p;
                rec.repetition_penalty = q.repetition_penalty; rec.presence_penalty = q.presence_penalty; rec.frequency_penalty = q.frequency_penalty;
                Compute::rocmCheck( mila_cdna4_sample_row_params_set( row_params_->rawData(), b, &rec, ctx_->getStream() ) );
            }
            row_requests_.assign( requests.begin(), requests.end() );
            row_request_vacant_.assign( requests.size(), 0 );
            row_request_draws_ = draws;
            if ( !row_masks_ )
            {
                row_masks_ = std::make_unique<TokenTensor>( ctx_->getDeviceId(), shape_t{ 2 * cfg_.max_batch } );
                for ( int b = 0; b < static_cast<int>( cfg_.max_batch ); ++b ) refreshRowMasks( b );
            }
        }
        /// setRowsRequests for ONE row, between steps (a request admitted into a retired row): the same checks, one record written through
        /// mila_cdna4_sample_row_params_set in stream order, the row's masks refreshed.  The first call after clearRowsRequests() turns the requests step on with
        /// every other row VACANT -- greedy and neutral on the device, and no part of the class facts until it gets a request of its own -- so ensureGraphRows
        /// re-captures only when the new record changes a class fact.  draws: as setRowsRequests' (kept when null).
        void setRowRequest( int b, const SamplingParams& q, const float* draws = nullptr )
        {
            requireRows( b );
            const std::string who = "GemmaTransformer::setRowRequest: row " + std::to_string( b );
            if ( !std::isfinite( q.temperature ) ) throw std::invalid_argument( who + ": temperature is not finite" );
            if ( q.top_k < 0 || !( q.top_p > 0.0f ) ) throw std::invalid_argument( who + ": need top_k >= 0, top_p > 0" );
            q.checkFilters( who.c_str() );
            if ( q.penalized() ) ensureTokenTable();
            auto record = []( const SamplingParams& s, float temperature )
            {
                mila_sample_row_params rec{};
                rec.temperature = temperature;
                rec.top_k = s.top_k; rec.top_p = s.top_p; rec.min_p = s.min_p;
                rec.repetition_penalty = s.repetition_penalty; rec.presence_penalty = s.presence_penalty; rec.frequency_penalty = s.frequency_penalty;
                return rec;
            };
            if ( !row_params_ )
            {
                row_params_ = std::make_unique<TokenTensor>( ctx_->getDeviceId(), shape_t{ static_cast<dim_t>( mila_cdna4_sample_row_params_bytes( static_cast<int>( cfg_.max_batch ) ) / 4 ) } );
                Compute::rocmCheck( mila_cdna4_memset_zero( row_params_->rawData(), row_params_->sizeInBytes(), ctx_->getStream() ) );
            }
            if ( row_requests_.empty() )      // the requests step turns on: every row vacant, as setRowsRequests leaves a row without a request
            {
                const mila_sample_row_params neutral = record( SamplingParams{}, 0.0f );
                for ( int r = 0; r < static_cast<int>( cfg_.max_batch ); ++r )
                    Compute::rocmCheck( mila_cdna4_sample_row_params_set( row_params_->rawData(), r, &neutral, ctx_->getStream() ) );
            }
            const mila_sample_row_params rec = record( q, q.temperature );
            Compute::rocmCheck( mila_cdna4_sample_row_params_set( row_params_->rawData(), b, &rec, ctx_->getStream() ) );
            if ( row_requests_.size() <= static_cast<size_t>( b ) )
            {
                row_requests_.resize( static_cast<size_t>( b ) + 1 );
                row_request_vacant_.resize( static_cast<size_t>( b ) + 1, 1 );
            }
            row_requests_[ static_cast<size_t>( b ) ] = q;
            row_request_vacant_[ static_cast<size_t>( b ) ] = 0;
            if ( draws ) row_request_draws_ = draws;
            if ( !row_masks_ )
            {
                row_masks_ = std::make_unique<TokenTensor>( ctx_->getDeviceId(), shape_t{ 2 * cfg_.max_batch } );
                for ( int r = 0; r < static_cast<int>( cfg_.max_batch ); ++r ) refreshRowMasks( r );
            }
            else refreshRowMasks( b );
        }
        /// A SHARED PREFILL: row `src`, directly after prefillRow( src, tokens, len, 0 ) and before any step, into the rows of dst_mask (bit r = row r) -- every
        /// layer's cache prefix [0, len) (one kv_rows_fork_layers_bf16 launch for all layers), the row's logits and the position word.  Afterwards a destination row is in
        /// exactly the state prefillRow( dst, the same tokens ) would have left it in: the same cache bits, logits bits and position.  Throws invalid_argument when
        /// row src's position word is not len (it was not prefilled with len tokens, or it has stepped: its logits are no longer the prefill's).
        /// On a ring model (GemmaConfig::bounded_local_kv_rows) the copy is every layer's LIVE BAND (one kv_rows_fork_layers_band_bf16 launch): afterwards a destination
        /// row holds, on every layer, the bits of every position a continuation from len can read -- [max( 0, len - window ), len) on the ring layers, [0, len) on the
        /// flat ones -- plus the logits and the position word; everything outside the band in the destination rows is left as it was, and the row's valid-from bound is
        /// max( 0, len - window + 1 ): beyond the window it cannot donate a shorter prefix, nor be rewound below len.
        void forkRow( int src, unsigned dst_mask, dim_t len )
        {
            requireRows( src );
            if ( dst_mask == 0 || ( dst_mask >> cfg_.max_batch ) != 0 || ( ( dst_mask >> src ) & 1u ) )
                throw std::invalid_argument( "GemmaTransformer::forkRow: dst_mask " + std::to_string( dst_mask ) + " must name rows of the model other than the source row " + std::to_string( src ) );
            if ( len < 1 || len > max_seq_ ) throw std::invalid_argument( "GemmaTransformer::forkRow: len " + std::to_string( len ) + " outside 1 .. " + std::to_string( max_seq_ ) );
            int32_t at = -1;
            Compute::rocmCheck( mila_cdna4_memcpy_d2h( &at, rows_->pos->data() + src, 4, ctx_->getStream() ) );
            ctx_->synchronize();
            if ( at != static_cast<int32_t>( len ) )
                throw std::invalid_argument( "GemmaTransformer::forkRow: row " + std::to_string( src ) + " is at position " + std::to_string( at ) + ", not " + std::to_string( len ) +
                                             " (a fork follows prefillRow( src, ..., len, 0 ) directly)" );
            forkLayers( src, dst_mask, len );
            const size_t V = static_cast<size_t>( cfg_.vocab_size );
            for ( int r = 0; r < static_cast<int>( cfg_.max_batch ); ++r )
            {
                if ( !( ( dst_mask >> r ) & 1u ) ) continue;
                Compute::rocmCheck( mila_cdna4_memcpy_d2d( rows_->logits->data() + static_cast<size_t>( r ) * V, rows_->logits->data() + static_cast<size_t>( src ) * V, V * 4, ctx_->getStream() ) );
                setRowWord( rows_->pos->data(), r, static_cast<int32_t>( len ) );
            }
        }
        /// A SHARED PREFIX: every layer's cache positions [0, len) of row `src` into the rows of dst_mask, and nothing else -- no logits, no position word: the
        /// prefillRow( dst, suffix, n - len, len ) that follows sets both.  Row src may be live, retired, and may have stepped: whatever sits at [0, len) of its
        /// caches is copied, and it must be at a position >= len (below it the caches hold nothing the row ever wrote).  One kv_rows_fork_layers_bf16 launch for all
        /// layers.  Refused (invalid_argument) before anything is enqueued: a one-row model, a mask that is empty, names src or a row outside the model, len < 1 or
        /// beyond the context; then the row's position word is read, and a len beyond it is refused as well.  On a ring model: the live band, as forkRow; refused as
        /// well is a len whose band the donor has already overwritten -- donor position - len > capacity - window, or a donor whose own valid-from bound lies above
        /// len - window (the rewind rule).
        void forkRowPrefix( int src, unsigned dst_mask, dim_t len )
        {
            if ( !rows_ || cfg_.max_batch <= 1 ) throw std::invalid_argument( "GemmaTransformer::forkRowPrefix: the model was built for one sequence (GemmaConfig::max_batch > 1)" );
            if ( src < 0 || src >= cfg_.max_batch ) throw std::invalid_argument( "GemmaTransformer::forkRowPrefix: source row " + std::to_string( src ) + " outside max_batch " + std::to_string( cfg_.max_batch ) );
            if ( dst_mask == 0 || ( dst_mask >> cfg_.max_batch ) != 0 || ( ( dst_mask >> src ) & 1u ) )
                throw std::invalid_argument( "GemmaTransformer::forkRowPrefix: dst_mask " + std::to_string( dst_mask ) + " must name rows of the model other than the source row " + std::to_string( src ) );
            if ( len < 1 || len > max_seq_ ) throw std::invalid_argument( "GemmaTransformer::forkRowPrefix: len " + std::to_string( len ) + " outside 1 .. " + std::to_string( max_seq_ ) );
            int32_t at = -1;
            Compute::rocmCheck( mila_cdna4_memcpy_d2h( &at, rows_->pos->data() + src, 4, ctx_->getStream() ) );
            ctx_->synchronize();
            if ( static_cast<int32_t>( len ) > at )
                throw std::invalid_argument( "GemmaTransformer::forkRowPrefix: len " + std::to_string( len ) + " beyond row " + std::to_string( src ) + "'s position " + std::to_string( at ) );
            if ( ringRows() )      // the rewind rule, on the donor: its writes up to `at` (and whatever came before a cut) must not have reused the band's cells
            {
                row_high_[ static_cast<size_t>( src ) ] = std::max<dim_t>( row_high_[ static_cast<size_t>( src ) ], at );
                if ( at - len > ring_capacity_ - cfg_.window || !rowHolds( src, len ) )
                    throw std::invalid_argument( "GemmaTransformer::forkRowPrefix: row " + std::to_string( src ) + " at position " + std::to_string( at ) + " (valid from " +
                                                 std::to_string( rowValidFrom( src ) ) + ") no longer holds the band of len " + std::to_string( len ) + " (ring capacity " +
                                                 std::to_string( ring_capacity_ ) + ", window " + std::to_string( cfg_.window ) + ")" );
            }
            forkLayers( src, dst_mask, len );
        }
        void clearRowsRequests() noexcept { row_requests_.clear(); row_request_vacant_.clear(); row_request_draws_ = nullptr; }
        bool rowsRequestsOn() const noexcept { return !row_requests_.empty(); }
        /// row b's bias table for the requests samplers (setTokenBias's arguments): written into the row's effective table, or -- when the row has an automaton --
        /// into the table its automaton composes from (set the automaton FIRST).  clearRowTokenBias: zeros.  stage / commit: the min_tokens restore of that row.
        void setRowTokenBias( int b, float fill, const int32_t* ids_host, const float* values_host, size_t n )
        {
            requireRows( b );
            if ( std::isnan( fill ) || ( std::isinf( fill ) && fill > 0.0f ) ) throw std::invalid_argument( "GemmaTransformer::setRowTokenBias: the fill value must be finite or -inf" );
            checkBiasEntries( ids_host, values_host, n, "GemmaTransformer::setRowTokenBias" );
            ensureRowBias();
            const bool automaton = row_automata_ && row_automata_->on( b );
            row_bias_->apply( b, automaton, fill, ids_host, values_host, n );
            if ( automaton ) row_automata_->compose( *row_bias_ );
            refreshRowMasks( b );
        }
        void clearRowTokenBias( int b )
        {
            requireRows( b );
            if ( !row_bias_ ) return;
            row_bias_->clear( b );
            if ( row_automata_ && row_automata_->on( b ) ) row_automata_->compose( *row_bias_ );
            refreshRowMasks( b );
        }
        void stageRowTokenBiasUpdate( int b, const int32_t* ids_host, const float* values_host, size_t n )
        {
            requireRows( b );
            if ( !row_bias_ || !row_bias_->on( b ) ) throw std::logic_error( "GemmaTransformer::stageRowTokenBiasUpdate: the row has no bias (setRowTokenBias)" );
            checkBiasEntries( ids_host, values_host, n, "GemmaTransformer::stageRowTokenBiasUpdate" );
            row_bias_->stage( b, ids_host, values_host, n );
        }
        void commitRowTokenBiasUpdate( int b )
        {
            requireRows( b );
            if ( !row_bias_ || !row_bias_->on( b ) ) throw std::logic_error( "GemmaTransformer::commitRowTokenBiasUpdate: the row has no bias (setRowTokenBias)" );
            row_bias_->commit( b );
            if ( row_automata_ && row_automata_->on( b ) ) row_automata_->compose( *row_bias_ );
        }
        /// row b's automaton: validated, uploaded, the state at its start, the row's effective table composed over zeros (a bias set afterwards composes again)
        void setRowTokenAutomaton( int b, const TokenAutomaton& a )
        {
            requireRows( b );
            a.validate( cfg_.vocab_size );
            ensureRowBias();
            if ( !row_automata_ ) row_automata_ = std::make_unique<Compute::RocmTokenAutomatonRows>( ctx_, cfg_.vocab_size, static_cast<int>( cfg_.max_batch ) );
            row_bias_->clear( b );
            row_automata_->set( b, a.class_of.data(), a.next.data(), a.num_states, a.num_classes, a.start );
            row_automata_->compose( *row_bias_ );
            refreshRowMasks( b );
        }
        void clearRowTokenAutomaton( int b )
        {
            requireRows( b );
            if ( !row_automata_ || !row_automata_->on( b ) ) return;
            row_automata_->clear( b );
            row_bias_->clear( b );
            refreshRowMasks( b );
        }
        std::optional<int32_t> rowTokenAutomatonState( int b )
        {
            requireRows( b );
            if ( !row_automata_ || !row_automata_->on( b ) ) return std::nullopt;
            return row_automata_->readState( b );
        }
        Compute::RocmTokenBiasRows* rowTokenBias() noexcept { return row_bias_.get(); }
        /// row b's next token from row b's logits through the ONE-ROW samplers with the row's request (a row's first token, from its prefill's logits; r: the row's
        /// draw, unused by a greedy row), then the row's automaton advanced by it
        void sampleRowRequest( int b, float r )
        {
            requireRows( b );
            if ( static_cast<size_t>( b ) >= row_requests_.size() || row_request_vacant_[ static_cast<size_t>( b ) ] ) throw std::invalid_argument( "GemmaTransformer::sampleRowRequest: row " + std::to_string( b ) + " has no request (setRowsRequests)" );
            const SamplingParams& q = row_requests_[ static_cast<size_t>( b ) ];
            const size_t V = static_cast<size_t>( cfg_.vocab_size );
            const float* logits = rows_->logits->data() + static_cast<size_t>( b ) * V;
            const float* bias = rowConstrained( b ) ? row_bias_->eff() + static_cast<size_t>( b ) * V : nullptr;
            const mila_sample_filters f = q.filters();
            uint32_t* words = tableWords( q, b, true );
            if ( q.temperature > 0.0f )
                Compute::rocmCheck( mila_cdna4_sample_radix_biased_fp32( logits, rows_->tok->data() + b, (int)cfg_.vocab_size, cfg_.final_logit_softcapping, q.temperature, q.top_k, q.top_p, r, &f,
                                                                         words, bias, 0, radix_scratch_->data(), radix_scratch_->sizeInBytes(), ctx_->getStream() ) );
            else
                Compute::rocmCheck( mila_cdna4_sample_argmax_biased_fp32( logits, rows_->tok->data() + b, (int)cfg_.vocab_size, cfg_.final_logit_softcapping, &f, words, bias, 0,
                                                                          sample_scratch_->data(), sample_scratch_->sizeInBytes(), ctx_->getStream() ) );
            if ( row_automata_ ) row_automata_->stepRow( *row_bias_, b, rows_->tok->data() + b );
        }
        void replayGraphRows()
        {
            if ( !rows_graph_exec_ ) throw std::runtime_error( "GemmaTransformer::replayGraphRows: captureGraphRows() first" );
            hipCheck( hipGraphLaunch( rows_graph_exec_, reinterpret_cast<hipStream_t>( ctx_->getStream() ) ), "hipGraphLaunch" );
        }
        size_t graphRowsCaptureCount() const noexcept { return rows_graph_captures_; }
        size_t graphRowsNodeCount() const
        {
            if ( !rows_graph_ ) return 0;
            size_t n = 0;
            hipCheck( hipGraphGetNodes( rows_graph_, nullptr, &n ), "hipGraphGetNodes" );
            return n;
        }

        // ------------------------------------------------------------------------------------
        // chain decode (GemmaConfig::draft_tokens > 0): one step over T = 2 .. draft_tokens + 1 CONSECUTIVE POSITIONS of the one sequence -- the last sampled token and
        // T - 1 drafted ones -- on the one KV cache: the rows step with the chain attention entry (mila_cdna4.h) in place of the rows attention, ended by
        // sample_argmax_chain_accept.  Row t's logits are bit-identical to decodeFused() at position + t given the same history; the accepted tokens are the greedy
        // ones.  A rejected draft leaves a stale cache row at its position, which the next step there overwrites before anything reads it.
        // With a bias table and / or a token automaton on (setTokenBias, setTokenAutomaton) the step is the constrained chain step: chain_compose as the first node
        // (an automaton), the layers, the biased chain tail over the logits (one table at stride 0, or the automaton's rows at stride vocab), chain_step as the last
        // node ahead of the log-probability launches.  One linear chain on one stream; the graph re-captures once per bias / automaton key.
        // ------------------------------------------------------------------------------------
        dim_t draftTokens() const noexcept { return cfg_.draft_tokens; }
        dim_t maxSeq() const noexcept { return max_seq_; }
        /// tokens[ 0 ] = the token about to be decoded, tokens[ 1 .. T - 1 ] = the drafts; row t is fed tokens[ t ]
        void setChainDrafts( const int32_t* tokens, int T )
        {
            requireChain();
            if ( T < 1 || T > cfg_.draft_tokens + 1 ) throw std::invalid_argument( "GemmaTransformer::setChainDrafts: 1 .. draft_tokens + 1 tokens" );
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( rows_->tok->data(), tokens, static_cast<size_t>( T ) * 4, ctx_->getStream() ) );
        }
        LogitsTensor& chainLogits() { requireChain(); return *rows_->logits; }
        /// {count, accepted tokens ...} of the last chain step (device; draft_tokens + 2 words)
        TokenTensor& chainResult() { requireChain(); return *rows_->result; }
        /// the position word the one-row graph and the chain step share, read back
        dim_t devicePosition()
        {
            int32_t p = 0;
            Compute::rocmCheck( mila_cdna4_memcpy_d2h( &p, pos_dev_->data(), 4, ctx_->getStream() ) );
            ctx_->synchronize();
            return p;
        }
        /// one eager chain step at `position` (the attention launches take the position by value; the tail advances the device position word, set here first)
        void decodeChain( int T, dim_t position )
        {
            checkChainStep( T, position );
            setDevicePosition( position );
            enqueueChainStepAndTail( T, bandBucket( position ), ChainAt{ static_cast<int>( position ), nullptr } );      // (checkChainStep: one bucket for all T rows)
            kv_fill_ = position + T;
        }
        /// capture the chain step for T rows from the device position word (set to start_position here, as captureGraph does)
        void captureGraphChain( int T, dim_t start_position )
        {
            checkChainStep( T, start_position );
            Compute::TraceRange tr( "gemma.captureGraphChain" );
            setDevicePosition( start_position );
            destroyGraphChain();
            hipStream_t s = reinterpret_cast<hipStream_t>( ctx_->getStream() );
            ctx_->synchronize();
            hipCheck( hipStreamBeginCapture( s, hipStreamCaptureModeThreadLocal ), "hipStreamBeginCapture" );
            hipGraph_t g = nullptr;
            const dim_t band = bandBucket( start_position );
            try { enqueueChainStepAndTail( T, band, ChainAt{ 0, pos_dev_->data() } ); }      // one linear chain on one stream, like the one-row graph
            catch ( ... ) { (void)hipStreamEndCapture( s, &g ); if ( g ) (void)hipGraphDestroy( g ); throw; }
            hipCheck( hipStreamEndCapture( s, &g ), "hipStreamEndCapture" );
            chain_graph_ = g;
            const hipError_t e = hipGraphInstantiate( &chain_graph_exec_, chain_graph_, nullptr, nullptr, 0 );
            if ( e != hipSuccess ) { chain_graph_exec_ = nullptr; destroyGraphChain(); hipCheck( e, "hipGraphInstantiate" ); }
            chain_captured_T_ = T; chain_captured_band_ = band;
            chain_captured_sampling_ = chain_sampling_; chain_captured_draws_ = chain_draws_;
            chain_captured_lp_ = step_lp_;
            chain_captured_bias_ = bias_on_; chain_captured_automaton_ = automatonKey();
            ++chain_graph_captures_;
        }
        /// capture on first use and whenever T or the live-length bucket changes; does NOT touch the device position word otherwise (the caller's loop owns it)
        void ensureGraphChain( int T, dim_t position )
        {
            checkChainStep( T, position );
            if ( !chain_graph_exec_ || chain_captured_T_ != T || chain_captured_band_ != bandBucket( position ) || chain_captured_lp_ != step_lp_ ||
                 !sameSampling( chain_captured_sampling_, chain_sampling_ ) || chain_captured_draws_ != chain_draws_ ||
                 chain_captured_bias_ != bias_on_ || chain_captured_automaton_ != automatonKey() )      // (a reset, a table update or an automaton of the same size: the same nodes)
                captureGraphChain( T, position );
        }
        /// speculative SAMPLING: with `sp` and `draws` set, a chain step verifies the drafts against SAMPLES instead of argmaxes -- the lm_head leaves the logits
        /// only, and the tail is mila_cdna4_sample_radix_chain_accept_fp32: row t samples s_t from its own logits at draws[ t ], and a draft is accepted exactly
        /// when it equals s_t.  With draws[ t ] the draw the one-row loop would use for that token, the emitted tokens are the one-row loop's (coupled draws).
        /// draws: device address of draft_tokens + 1 floats of host-visible memory.  nullopt / nullptr = the greedy chain step.  Eager decodeChain follows the
        /// setter at once; ensureGraphChain() re-captures when either changes.
        void setChainSampling( const std::optional<SamplingParams>& sp, const float* draws )
        {
            requireChain();
            if ( sp && !( sp->temperature > 0.0f ) ) throw std::invalid_argument( "GemmaTransformer::setChainSampling: temperature must be > 0 (greedy: the greedy chain step)" );
            // row t of a chain step would need the token table plus the drafts 1 .. t: not built; refused rather than silently unfiltered
            if ( sp && sp->filtered() ) throw std::invalid_argument( "GemmaTransformer::setChainSampling: the chain step takes no sampling filters" );
            chain_sampling_ = sp; chain_draws_ = draws;
        }
        void replayGraphChain()
        {
            if ( !chain_graph_exec_ ) throw std::runtime_error( "GemmaTransformer::replayGraphChain: captureGraphChain() first" );
            hipCheck( hipGraphLaunch( chain_graph_exec_, reinterpret_cast<hipStream_t>( ctx_->getStream() ) ), "hipGraphLaunch" );
        }
        size_t graphChainCaptureCount() const noexcept { return chain_graph_captures_; }
        size_t graphChainNodeCount() const
        {
            if ( !chain_graph_ ) return 0;
            size_t n = 0;
            hipCheck( hipGraphGetNodes( chain_graph_, nullptr, &n ), "hipGraphGetNodes" );
            return n;
        }
        int graphChainRows() const noexcept { return chain_graph_exec_ ? chain_captured_T_ : 0; }

        /// greedy device sampler: token <- argmax(logits); the token never leaves the device
        /// (GemmaModel::enqueueSampleNext, Models/GemmaModel.ixx:568)
        void sampleGreedy( TokenTensor& token_out ) { sampleGreedyWith( token_out, filters_ ); }
        /// ... with the penalties of `fl` (setSamplingFilters()'s by default): argmax of the adjusted logits, counted in row 0 of the token table
        void sampleGreedyWith( TokenTensor& token_out, const SamplingParams& fl )
        {
            Compute::TraceRange tr( "gemma.sample(greedy)" );
            if ( fl.penalized() || bias_on_ || automaton_on_ )
            {
                const mila_sample_filters f = fl.filters();
                Compute::rocmCheck( mila_cdna4_sample_argmax_biased_fp32( logits_->data(), token_out.data(), (int)cfg_.vocab_size, cfg_.final_logit_softcapping, &f,
                                                                          tableWords( fl, 0, true ), samplerBias(), 0, sample_scratch_->data(), sample_scratch_->sizeInBytes(),
                                                                          ctx_->getStream() ) );
                if ( automaton_on_ ) token_automaton_->step( biasValues(), token_out.data() );      // the launch a captured step holds behind its tail
                return;
            }
            Compute::rocmCheck( mila_cdna4_sample_argmax_fp32( logits_->data(), token_out.data(), (int)cfg_.vocab_size, sample_scratch_->data(),
                                                               sample_scratch_->sizeInBytes(), ctx_->getStream() ) );
        }

        /// token <- a draw from softmax(softcap(logits) / temperature) restricted by top-k / top-p; the Gemma final logit
        /// softcap (cfg.final_logit_softcapping) is applied here, at the sampler (Gemma.ixx:30-32)
        void sampleStochastic( TokenTensor& token_out, const SamplingParams& sp, float r )
        {
            if ( sp.temperature <= 0.0f ) { sampleGreedy( token_out ); return; }
            Compute::TraceRange tr( "gemma.sample(stochastic)" );
            if ( bias_on_ || automaton_on_ ) throw std::invalid_argument( "GemmaTransformer::sampleStochastic: the search pipeline takes no bias table (sampleStochasticRadix)" );
            const size_t need = mila_cdna4_sample_stochastic_scratch_bytes( (int)cfg_.vocab_size );
            void* scratch = ctx_->getScratch( need );
            Compute::rocmCheck( mila_cdna4_sample_stochastic_fp32( logits_->data(), token_out.data(), (int)cfg_.vocab_size, cfg_.final_logit_softcapping, sp.temperature,
                                                                   sp.top_k, sp.top_p, r, scratch, need, ctx_->getStream() ) );
        }

        /// sampleStochastic through the radix pipeline (fewer launches, a model-owned workspace): the eager form of what a stochastic captured step ends with
        void sampleStochasticRadix( TokenTensor& token_out, const SamplingParams& sp, float r )
        {
            if ( sp.temperature <= 0.0f ) { sampleGreedyWith( token_out, sp.filtered() ? sp : filters_ ); return; }
            Compute::TraceRange tr( "gemma.sample(stochastic, radix)" );
            if ( sp.filtered() || bias_on_ || automaton_on_ )      // the eager form of what a filtered / biased / constrained captured step ends with
            {
                sp.checkFilters( "GemmaTransformer::sampleStochasticRadix" );
                const mila_sample_filters f = sp.filters();
                Compute::rocmCheck( mila_cdna4_sample_radix_biased_fp32( logits_->data(), token_out.data(), (int)cfg_.vocab_size, cfg_.final_logit_softcapping, sp.temperature, sp.top_k,
                                                                         sp.top_p, r, &f, tableWords( sp, 0, true ), samplerBias(), 0, radix_scratch_->data(), radix_scratch_->sizeInBytes(),
                                                                         ctx_->getStream() ) );
                if ( automaton_on_ ) token_automaton_->step( biasValues(), token_out.data() );
                return;
            }
            Compute::rocmCheck( mila_cdna4_sample_radix_fp32( logits_->data(), token_out.data(), (int)cfg_.vocab_size, cfg_.final_logit_softcapping, sp.temperature, sp.top_k, sp.top_p, r,
                                                              radix_scratch_->data(), radix_scratch_->sizeInBytes(), ctx_->getStream() ) );
        }

        // ------------------------------------------------------------------------------------
        // prefill: whole prompt as one chunk (288 GB: no 12 GB-card chunking);
        // logits for the last position only (Gemma.ixx:269-276)
        // ------------------------------------------------------------------------------------
        LogitsTensor& prefill( const TokenTensor& tokens, dim_t T, dim_t position_offset = 0 )
        {
            if ( T <= 0 || T > max_prefill_ ) throw std::invalid_argument( "GemmaTransformer::prefill: chunk length out of range" );
            Compute::TraceRange tr( "gemma.prefill" );
            checkPosition( position_offset, T );
            return prefillTail( *prefillBlocks( tokens, T, position_offset ), T );
        }

        /// prefill() that also SCORES the chunk: after the same blocks (every route, the FP8 KV cache, the bounded local KV, any cache row) the final norm runs over
        /// rows [first_row, T) of the last block's output and the scoring lm_head (RocmLmHeadScoreOp) over them: row r reports the log-probability of targets_dev[ r ]
        /// (one device word per row of the chunk, -1 = none) and, with argmax, the greedy token and its log-probability; read them with scoreOp().read( T - first_row, .. ).
        /// The last row's logits are left in logits() as prefill() leaves them.  Nothing synchronizes.
        LogitsTensor& prefillScored( const TokenTensor& tokens, dim_t T, dim_t position_offset, const int32_t* targets_dev, dim_t first_row = 0, bool argmax = true )
        {
            if ( T <= 0 || T > max_prefill_ ) throw std::invalid_argument( "GemmaTransformer::prefillScored: chunk length out of range" );
            if ( first_row < 0 || first_row >= T ) throw std::invalid_argument( "GemmaTransformer::prefillScored: first_row outside the chunk" );
            if ( !targets_dev ) throw std::invalid_argument( "GemmaTransformer::prefillScored: targets are required" );
            Compute::TraceRange tr( "gemma.prefill_scored" );
            checkPosition( position_offset, T );
            TensorType& x = *prefillBlocks( tokens, T, position_offset );
            const dim_t D = cfg_.embedding_dim, rows = T - first_row;
            if ( !score_op_ )
                score_op_ = std::make_unique<Compute::RocmLmHeadScoreOp>( ctx_, Compute::LmHeadScoreOpConfig{ cfg_.vocab_size, D, cfg_.final_logit_softcapping, max_prefill_ } );
            // pf_norm_ is free once the last block has run (the tails write the NEXT block's input norm there)
            final_norm_->getOperation().forwardRows( x.data() + static_cast<size_t>( first_row * D ), pf_norm_->data(), static_cast<int>( rows ) );
            const float* sc = nullptr;
            if constexpr ( kTableFmt != 0 ) sc = lm_head_->getWeightScale()->data();
            score_op_->forward( pf_norm_->data(), static_cast<size_t>( D ), lm_head_->getWeight().rawData(), sc, kTableFmt, targets_dev + first_row, rows, argmax );
            return prefillTail( x, T );
        }
        Compute::RocmLmHeadScoreOp& scoreOp()
        {
            if ( !score_op_ ) throw std::logic_error( "GemmaTransformer::scoreOp: prefillScored() first" );
            return *score_op_;
        }

    private:
        /// the tail every prefill route shares: the final norm of the chunk's last row and the lm_head on it
        LogitsTensor& prefillTail( TensorType& x, dim_t T )
        {
            const dim_t D = cfg_.embedding_dim;
            auto last = x.slice( static_cast<size_t>( ( T - 1 ) * D ), shape_t{ 1, 1, D } );
            auto& normed = final_norm_->forward( last );
            head( normed.data() );
            return *logits_;
        }
        /// the blocks of a prefill chunk by the route prefill() takes; the last block's output [T, D]
        TensorType* prefillBlocks( const TokenTensor& tokens, dim_t T, dim_t position_offset )
        {
            kv_fill_ = position_offset + T;
            const dim_t D = cfg_.embedding_dim;
            embed( tokens.data(), static_cast<int>( T ), *pf_x_[ 0 ] );
            TensorType* x = pf_x_[ 0 ].get();
            const bool fused = fused_prefill_ && fusedPrefillApplicable();
            if ( fused && prefill_overlap_ && overlapApplicable( T ) ) return prefillOverlapped( tokens, T, position_offset );
            int flip = 0;
            bool q8_normed = false;
            for ( size_t i = 0; i < layers_.size(); ++i )
            {
                Layer& L = layers_[ i ];
                if ( !fused ) { x = &L.prefill( x->view( shape_t{ 1, T, D } ), position_offset ); continue; }   // GemmaBlock::prefill, one component per step
                // one call over rows [0, T), the Linears writing their components' pooled outputs; the first block's input norm is its component's forward, every later
                // one was written into pf_norm_ by the tail before it
                BlockRows r{ 0, static_cast<int>( T ), x, pf_x_[ 1 - flip ].get(), i ? pf_norm_.get() : &L.input_norm->forward( x->view( shape_t{ 1, T, D } ) ),
                             ws_qkv_.get(), ws_o_.get(), ws_gate_up_.get(), ws_down_.get(), q8_normed };
                q8_normed = blockPrefillFused( L, i + 1 < layers_.size() ? &layers_[ i + 1 ] : nullptr, r, static_cast<int>( position_offset ) );
                x = r.out;
                flip = 1 - flip;
            }
            return x;
        }
    public:

        /// algorithmic bytes one decode token must read: weights + scales + norm weights + KV band
        double decodeBytesPerToken( dim_t context ) const
        {
            double b = 0;
            for ( auto& L : layers_ )
            {
                b += L.qkv_proj->getParameterBytes() + L.o_proj->getParameterBytes() + L.fc_gate_up->getParameterBytes() + L.fc_down->getParameterBytes();
                const dim_t band = L.global ? context : std::min<dim_t>( context, cfg_.window );
                b += cfg_.kv_fp8 ? 2.0 * band * cfg_.numKvHeads( L.global ) * ( cfg_.headDim( L.global ) + 4 ) : 2.0 * band * cfg_.kvWidth( L.global ) * 2;
                b += 2.0 * ( 4 * cfg_.embedding_dim + 2 * cfg_.headDim( L.global ) );
            }
            b += lm_head_->getParameterBytes();
            return b;
        }
        double weightBytes() const
        {
            double b = lm_head_->getParameterBytes();
            for ( auto& L : layers_ ) b += L.qkv_proj->getParameterBytes() + L.o_proj->getParameterBytes() + L.fc_gate_up->getParameterBytes() + L.fc_down->getParameterBytes();
            return b;
        }
        /// GemmaTransformer::rewindKvCache (Gemma.ixx): every block drops positions >= `position`; false when any block refuses (a bounded ring
        /// that has already evicted what the rewind would need) -- the caller then prefills from 0, which overwrites positionally
        bool rewindKvCache( dim_t position, dim_t written )
        {
            if ( position < 0 || position > written ) return false;
            bool ok = true;
            for ( auto& L : layers_ ) ok = L.rewindKvCache( position, written ) && ok;
            if ( ok ) kv_fill_ = position;
            return ok;
        }
        /// the same against the fill this transformer has tracked itself (prefill / decode / decodeFused calls; graph replays advance on the device, so a
        /// caller that replays -- GemmaModel -- passes the fill explicitly): positions beyond the fill are rejected (Gemma.Cuda.cpp:373-383)
        bool rewindKvCache( dim_t position ) { return rewindKvCache( position, kv_fill_ ); }
        dim_t kvFill() const noexcept { return kv_fill_; }
        /// incremental prefill (prompt-prefix reuse): positions [0, offset) stay resident, tokens [offset, T) are prefilled at their positions, in chunks of
        /// the built prefill size; logits of the last position (Gemma.ixx prefillFrom; Gemma.Cuda.cpp:338-391)
        LogitsTensor& prefillFrom( const TokenTensor& tokens, dim_t T, dim_t offset )
        {
            if ( offset < 0 || offset >= T ) throw std::invalid_argument( "GemmaTransformer::prefillFrom: offset " + std::to_string( offset ) + " outside the prompt of " + std::to_string( T ) + " tokens" );
            LogitsTensor* out = nullptr;
            for ( dim_t p0 = offset; p0 < T; p0 += max_prefill_ )
            {
                const dim_t n = std::min( max_prefill_, T - p0 );
                auto chunk = tokens.slice( static_cast<size_t>( p0 ), shape_t{ 1, n } );
                out = &prefill( chunk, n, p0 );
            }
            return *out;
        }
        void resetKVCache() { for ( auto& L : layers_ ) L.resetKVCache(); }
        LmHeadLinearType& lmHead() { return *lm_head_; }
        RmsNormType& finalNorm() { return *final_norm_; }
        TokenEmbeddingType& tokenEmbedding() { return *temb_; }

        double gateUpBytes( size_t i ) const { return static_cast<double>( layers_[ i ].fc_gate_up->getParameterBytes() ); }
        /// launch only the dominant decode kernel of the schedule, the fc_gate_up fused matvec of layer i -- used by the bench to time that kernel with HIP events on
        /// the model stream
        void launchDominant( size_t i )
        {
            if ( !cur_hidden_ ) cur_hidden_ = hidden_[ 0 ]->data();   // no fused step has run yet (reference-order timing)
            fusedGateUp( layers_[ i % layers_.size() ] );
        }
        double dominantBytes( size_t i ) const { return gateUpBytes( i % layers_.size() ); }

    private:
        void destroyGraph() noexcept
        {
            if ( graph_exec_ ) (void)hipGraphExecDestroy( graph_exec_ );
            if ( graph_ ) (void)hipGraphDestroy( graph_ );
            graph_exec_ = nullptr; graph_ = nullptr; captured_token_ = nullptr;
        }
        void fill( uint16_t* dst, dim_t n, uint64_t seed, float amp, float offset )
        {
            Compute::rocmCheck( mila_cdna4_fill_uniform_bf16( dst, n, seed, amp, offset, ctx_->getStream() ) );
        }

        template<typename C, typename... A> std::shared_ptr<C> make( const std::string& name, A&&... a )
        {
            auto c = std::make_shared<C>( name, std::forward<A>( a )... );
            c->setExecutionContext( ctx_ );
            return c;
        }

        void buildAll()
        {
            const dim_t D = cfg_.embedding_dim, P = max_prefill_;
            const auto dev = ctx_->getDeviceId();
            auto rms = [&]( dim_t dim ) { return RmsNormConfig( dim ).withEpsilon( cfg_.rms_norm_eps ).withBias( false ); };
            // workspace every block shares (they run one after the other): split scratch, attention / GeGLU / residual outputs, two stream buffers
            const dim_t maxq = std::max( cfg_.qWidth( false ), cfg_.qWidth( true ) ), maxkv = std::max( cfg_.kvWidth( false ), cfg_.kvWidth( true ) );
            q_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, maxq } );
            k_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, maxkv } );
            v_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, maxkv } );
            attn_out_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, maxq } );
            res1_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, D } );
            res2_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, D } );
            geglu_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, cfg_.hidden_dim } );
            for ( int i = 0; i < 2; ++i ) blk_out_[ i ] = std::make_shared<TensorType>( dev, shape_t{ 1, P, D } );
            // ... and one output buffer per component ROLE, shared by that role's component in every block (blocks run one after the other): the reference's pooled block
            // workspace (Gemma.ixx allocateBlockWorkspace: normed, qkv, q/k/v_normed, o, o_normed, ffn_in, gate_up, ffn_down, ffn_normed).  Per layer only the KV caches
            // and the parameters remain (Tests/.../Gemma.Cuda.cpp:494 StateMemory_PerLayerSlopeIsKvCacheNotActivations).
            const dim_t maxpacked = std::max( cfg_.packedQkvWidth( false ), cfg_.packedQkvWidth( true ) );
            ws_normed_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, D } );
            ws_o_normed_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, D } );
            ws_ffn_in_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, D } );
            ws_ffn_normed_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, D } );
            ws_q_normed_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, maxq } );
            ws_k_normed_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, maxkv } );
            ws_v_normed_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, maxkv } );
            ws_qkv_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, maxpacked } );
            ws_o_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, D } );
            ws_gate_up_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, 2 * cfg_.hidden_dim } );
            ws_down_ = std::make_shared<TensorType>( dev, shape_t{ 1, P, D } );
            for ( dim_t i = 0; i < cfg_.num_layers; ++i )
            {
                const std::string n = name_ + ".tf_layer_" + std::to_string( i );
                const bool g = cfg_.isGlobalLayer( i );
                GemmaBlockConfig bc;
                bc.model_dim = D; bc.hidden_dim = cfg_.hidden_dim; bc.num_heads = cfg_.num_heads; bc.num_kv_heads = cfg_.numKvHeads( g ); bc.head_dim = cfg_.headDim( g );
                bc.window = cfg_.windowFor( g ); bc.rotary_dim = g ? cfg_.global_rotary_dim : 0; bc.rope_theta = g ? cfg_.rope_theta_global : cfg_.rope_theta_local;
                bc.rms_norm_eps = cfg_.rms_norm_eps; bc.max_seq = max_seq_;
                // KV policy (Quantization/KvCache policies; CudaGqaOp.ixx:552-574): 288 GB of HBM makes unbounded caches the default;
                // SlidingWindowKvCache bounds the sliding-window layers to window + prefill_chunk - 1 rows, global layers stay unbounded
                auto wire = [&]( auto block )
                {
                    block->setExecutionContext( ctx_ );
                    block->installSharedWorkspace( q_, k_, v_, blk_out_[ i & 1 ] );
                    block->attn->installSharedOutput( attn_out_ );
                    block->geglu->installSharedOutput( geglu_ );
                    block->res_1->installSharedOutput( res1_ );
                    block->res_2->installSharedOutput( res2_ );
                    block->input_norm->installSharedOutput( ws_normed_ ); block->post_attn_norm->installSharedOutput( ws_o_normed_ );
                    block->pre_ffn_norm->installSharedOutput( ws_ffn_in_ ); block->post_ffn_norm->installSharedOutput( ws_ffn_normed_ );
                    block->q_norm->installSharedOutput( ws_q_normed_ ); block->k_norm->installSharedOutput( ws_k_normed_ ); block->v_norm->installSharedOutput( ws_v_normed_ );
                    block->qkv_proj->installSharedOutput( ws_qkv_ ); block->o_proj->installSharedOutput( ws_o_ );
                    block->fc_gate_up->installSharedOutput( ws_gate_up_ ); block->fc_down->installSharedOutput( ws_down_ );
                    block->build( BuildContext( shape_t{ 1, P, D }, RuntimeMode::Inference ) );
                    layers_.push_back( block );
                };
                if ( cfg_.kv_fp8 && g ) wire( std::make_shared<KvFp8GlobalBlockType>( n, bc ) );
                else if ( cfg_.kv_fp8 ) wire( std::make_shared<KvFp8LocalBlockType>( n, bc ) );
                else if ( g ) wire( std::make_shared<GlobalBlockType>( n, bc ) );
                else if ( cfg_.bounded_local_kv ) wire( std::make_shared<BoundedLocalBlockType>( n, bc ) );
                else wire( std::make_shared<LocalBlockType>( n, bc ) );
            }
            // TokenEmbedding owns the raw table; the tied head adopts it before its build, so it never allocates its own (Gemma.ixx:659-684)
            temb_ = make<TokenEmbeddingType>( name_ + ".temb", TokenEmbeddingConfig().withVocabSize( cfg_.vocab_size ).withEmbeddingDim( D ).withEmbeddingScale( cfg_.embeddingScale() ) );
            temb_->build( BuildContext( shape_t{ 1, P }, RuntimeMode::Inference ) );
            final_norm_ = make<RmsNormType>( name_ + ".rmsn_final", rms( D ) );
            final_norm_->build( BuildContext( shape_t{ 1, 1, D }, RuntimeMode::Inference ) );
            lm_head_ = make<LmHeadLinearType>( name_ + ".lm_head", LinearConfig( D, cfg_.vocab_size ).withBias( false ) );
            if constexpr ( TableQuantizationPolicy::kIsQuantized ) lm_head_->installSharedWeight( temb_->getWeightTensorShared(), temb_->getWeightScalesTensorShared() );
            else lm_head_->installSharedWeight( temb_->getWeightTensorShared() );
            lm_head_->build( BuildContext( shape_t{ 1, 1, D }, RuntimeMode::Inference ) );

            for ( int i = 0; i < 3; ++i ) hidden_[ i ] = std::make_unique<TensorType>( dev, shape_t{ 1, 1, D } );
            for ( int i = 0; i < 2; ++i ) pf_x_[ i ] = std::make_unique<TensorType>( dev, shape_t{ 1, P, D } );
            pf_norm_ = std::make_unique<TensorType>( dev, shape_t{ 1, P, D } );
            pf_norm2_ = std::make_unique<TensorType>( dev, shape_t{ 1, P, D } );
            if constexpr ( kFmt != 0 )      // per-token e4m3 rows + scales of the fp8 x fp8 prefill paths (W4A8; W8A8 when the fp8 policy opts in)
                for ( int i = 0; i < 2; ++i )
                {
                    pf_q8_[ i ] = std::make_unique<TensorType>( dev, shape_t{ 1, P, ( D + 1 ) / 2 } );
                    pf_ts_[ i ] = std::make_unique<LogitsTensor>( dev, shape_t{ P } );
                }
            f_qkv_ = std::make_unique<TensorType>( dev, shape_t{ std::max( cfg_.packedQkvWidth( false ), cfg_.packedQkvWidth( true ) ) } );
            f_q_ = std::make_unique<TensorType>( dev, shape_t{ std::max( cfg_.qWidth( false ), cfg_.qWidth( true ) ) } );
            f_o_ = std::make_unique<TensorType>( dev, shape_t{ D } );
            f_down_ = std::make_unique<TensorType>( dev, shape_t{ D } );
            f_act_ = std::make_unique<TensorType>( dev, shape_t{ cfg_.hidden_dim } );
            logits_ = std::make_unique<LogitsTensor>( dev, shape_t{ 1, 1, cfg_.vocab_size } );
            pos_dev_ = std::make_unique<TokenTensor>( dev, shape_t{ 1 } );
            sample_scratch_ = std::make_unique<LogitsTensor>( dev, shape_t{ static_cast<dim_t>( mila_cdna4_sample_scratch_bytes() / 4 ) } );
            // split-attention partials of the fused / graph decode step: model-owned and never re-allocated (see captureGraph)
            attn_partials_ = std::make_unique<LogitsTensor>( dev, shape_t{ static_cast<dim_t>( ( attnScratchBytes() + 3 ) / 4 ) } );
            // the radix sampler's workspace: model-owned for the same reason (a captured stochastic step's nodes point into it)
            radix_scratch_ = std::make_unique<LogitsTensor>( dev, shape_t{ static_cast<dim_t>( ( mila_cdna4_sample_radix_scratch_bytes( (int)cfg_.vocab_size ) + 3 ) / 4 ) } );
            if ( cfg_.max_batch > 1 || cfg_.draft_tokens > 0 ) buildRows();
            ctx_->synchronize();
        }

        void checkPosition( dim_t position, dim_t n ) const
        {
            if ( position < 0 || position + n > max_seq_ ) throw std::invalid_argument( "GemmaTransformer: position beyond the built sequence length" );
        }
        size_t attnScratchBytes() const
        {
            return std::max( mila_cdna4_attn_decode_scratch_bytes( 1, (int)cfg_.num_heads, (int)cfg_.head_dim ),
                             mila_cdna4_attn_decode_scratch_bytes( 1, (int)cfg_.num_heads, (int)cfg_.global_head_dim ) );
        }

        /// TokenEmbedding's gather (bf16 table, or FP8 table x row scale) and scale(sqrt(D)), token ids on the device
        void embed( const int32_t* tokens_dev, int n, TensorType& out ) { temb_->gather( tokens_dev, n, out ); }

        /// lm_head on the normalized last hidden state, fp32 logits (the 1e-3 bar is asserted on fp32)
        void head( const uint16_t* normed )
        {
            const float* sc = nullptr;
            if constexpr ( kTableFmt != 0 ) sc = lm_head_->getWeightScale()->data();
            Compute::rocmCheck( mila_cdna4_matvec_f32out( logits_->data(), normed, lm_head_->getWeight().rawData(), sc, kTableFmt, (int)cfg_.embedding_dim,
                                                          (int)cfg_.vocab_size, 0, ctx_->getStream() ) );
        }

        // ---- fused-glue prefill (the reference-order path is GemmaBlock::prefill) -----------------------
        /// What one call of blockPrefillFused() works on: rows [row0, row0 + rows) of the chunk.  The one-stream prefill passes the whole chunk and the components'
        /// pooled outputs; the two-stream form passes each half, buffers of its own, and the event that orders the halves' attention.
        struct BlockRows
        {
            int row0, rows;
            TensorType *x, *out;                      ///< the block's input and output rows (the two pf_x_ buffers, alternating)
            TensorType* normed;                       ///< input_norm( x )
            TensorType *qkv, *o, *gate_up, *ffn;      ///< where qkv_proj, o_proj, fc_gate_up (when it runs unfused) and fc_down write
            bool q8_normed = false;                   ///< the tail before this block left `normed`'s rows in pf_q8_[ 1 ] / pf_ts_[ 1 ] as well, quantized per token
            hipEvent_t kv_record = nullptr;           ///< recorded once this call's K / V rows are in the cache ...
            hipEvent_t kv_wait = nullptr;             ///< ... and what its attention waits for: the K / V rows of the chunk's earlier rows, written on another stream
        };

        /// GemmaBlock::forward with the glue fused (bit-identical to GemmaBlock::prefill): the packed qkv rows go straight through q/k/v norm + RoPE into q and the
        /// KV cache (no split3 / kv_write), and each sandwich tail (RmsNorm + Residual (+ layer scalar) + the next RmsNorm) is one launch.  `nextL`: the block whose
        /// input_norm the second tail applies, into pf_norm_.  Returns whether that tail wrote those rows quantized per token as well: the next call's q8_normed.
        bool blockPrefillFused( Layer& L, Layer* nextL, const BlockRows& r, int position_offset )
        {
            const bool g = L.global;
            const dim_t NH = cfg_.num_heads, NKV = cfg_.numKvHeads( g ), HD = cfg_.headDim( g ), D = cfg_.embedding_dim, F = cfg_.hidden_dim;
            const int T = r.rows, position = position_offset + r.row0;
            mila_stream_t st = ctx_->getStream();
            // a call's region of a buffer starts at its first row in the buffer's OWN (widest) row pitch: the first half of a chunk may run a layer of the other kind
            // (wider q / qkv rows) ahead of the second half, and the regions of the two must not meet whatever the widths
            auto rows = [&]( TensorType& t, dim_t width ) { return t.slice( static_cast<size_t>( r.row0 ) * static_cast<size_t>( t.shape().back() ), shape_t{ 1, T, width } ); };
            auto x3 = rows( *r.x, D ), out = rows( *r.out, D ), normed = rows( *r.normed, D ), next_normed = rows( *pf_norm_, D );
            // per-token e4m3 rows + scales a tail hands to the Linear behind it: [ 0 ] pre_ffn_norm's for fc_gate_up, [ 1 ] the next block's input_norm's for its qkv_proj
            uint8_t* q8[ 2 ] = { nullptr, nullptr };
            float* ts8[ 2 ] = { nullptr, nullptr };
            if constexpr ( kFmt != 0 )
                for ( int i = 0; i < 2; ++i )
                {
                    q8[ i ] = static_cast<uint8_t*>( pf_q8_[ i ]->rawData() ) + static_cast<size_t>( r.row0 ) * static_cast<size_t>( D );
                    ts8[ i ] = pf_ts_[ i ]->data() + r.row0;
                }
            auto qkv = rows( *r.qkv, cfg_.packedQkvWidth( g ) );
            // the tail before this block wrote `normed` quantized as well -- the Linear's own quantization launch is skipped (same bits)
            if ( r.q8_normed ) L.qkv_proj->getOperation().forwardFp8Activations( q8[ 1 ], ts8[ 1 ], qkv.data(), T );
            else L.qkv_proj->getOperation().forward( normed, qkv );
            auto q = rows( *q_, NH * HD );
            const uint16_t* qp = qkv.data();
            const uint16_t* kp = qp + (size_t)( NH * HD );
            const uint16_t* vp = g ? kp : kp + (size_t)( NKV * HD );
            if ( L.kvFp8() )      // the same launch with the quantizing append; prefillFromCache() is then the policy's attention-only prefill (band dequant + the bf16 flash kernels)
                Compute::rocmCheck( mila_cdna4_fused_qkv_post_kvfp8_prefill( q.data(), L.keyCacheFp8(), L.valueCacheFp8(), L.keyScales(), L.valueScales(), qp, kp, vp,
                                                                             (int64_t)cfg_.packedQkvWidth( g ), L.q_norm->getWeight()->data(), L.k_norm->getWeight()->data(),
                                                                             L.v_norm->getWeight()->data(), L.rope->cosCache(), L.rope->sinCache(), T, (int)NH, (int)NKV, (int)HD,
                                                                             position, (int)L.cacheCapacity(), cfg_.rms_norm_eps, st ) );
            else
                Compute::rocmCheck( mila_cdna4_fused_qkv_post_prefill( q.data(), L.keyCache(), L.valueCache(), qp, kp, vp, (int64_t)cfg_.packedQkvWidth( g ),
                                                                       L.q_norm->getWeight()->data(), L.k_norm->getWeight()->data(), L.v_norm->getWeight()->data(),
                                                                       L.rope->cosCache(), L.rope->sinCache(), T, (int)NH, (int)NKV, (int)HD, position,
                                                                       (int)L.cacheCapacity(), cfg_.rms_norm_eps, st ) );
            if ( r.kv_record ) hipCheck( hipEventRecord( r.kv_record, reinterpret_cast<hipStream_t>( st ) ), "hipEventRecord" );
            if ( r.kv_wait ) hipCheck( hipStreamWaitEvent( reinterpret_cast<hipStream_t>( st ), r.kv_wait, 0 ), "hipStreamWaitEvent" );
            auto attn = rows( *attn_out_, NH * HD );
            L.prefillFromCache( q, attn, T, position );
            auto o = rows( *r.o, D );
            L.o_proj->getOperation().forward( attn, o );
            auto res1 = rows( *res1_, D ), ffn_in = rows( *pf_norm2_, D );
            // W4A8 / W8A8: a tail whose normalised rows feed a Linear on the fp8 x fp8 path writes them quantized per token as well (fused_tail_norm_quant)
            auto& gate_up_op = L.fc_gate_up->getOperation();
            const bool q8_ffn = gate_up_op.gegluWantsFp8Rows( T ), q8_next = nextL && nextL->qkv_proj->getOperation().acceptsFp8Activations( T );
            if ( q8_ffn )
                Compute::rocmCheck( mila_cdna4_fused_tail_norm_quant_bf16( res1.data(), ffn_in.data(), q8[ 0 ], ts8[ 0 ], o.data(), x3.data(), L.post_attn_norm->getWeight()->data(),
                                                                           L.pre_ffn_norm->getWeight()->data(), T, (int)D, 1.0f, cfg_.rms_norm_eps, st ) );
            else
                Compute::rocmCheck( mila_cdna4_fused_tail_norm_bf16( res1.data(), ffn_in.data(), o.data(), x3.data(), L.post_attn_norm->getWeight()->data(),
                                                                     L.pre_ffn_norm->getWeight()->data(), T, (int)D, 1.0f, cfg_.rms_norm_eps, st ) );
            auto act = rows( *geglu_, F );
            auto gate_up = rows( *r.gate_up, 2 * F );         // only written where no fused Linear + GeGLU serves this [T, D, F]
            gate_up_op.forwardGeglu( ffn_in, act, gate_up, q8_ffn ? q8[ 0 ] : nullptr, q8_ffn ? ts8[ 0 ] : nullptr );
            auto ffn = rows( *r.ffn, D );
            L.fc_down->getOperation().forward( act, ffn );
            if ( q8_next )
                Compute::rocmCheck( mila_cdna4_fused_tail_norm_quant_bf16( out.data(), next_normed.data(), q8[ 1 ], ts8[ 1 ], ffn.data(), res1.data(), L.post_ffn_norm->getWeight()->data(),
                                                                           nextL->input_norm->getWeight()->data(), T, (int)D, L.layer_scalar, cfg_.rms_norm_eps, st ) );
            else
                Compute::rocmCheck( mila_cdna4_fused_tail_norm_bf16( out.data(), nextL ? next_normed.data() : nullptr, ffn.data(), res1.data(), L.post_ffn_norm->getWeight()->data(),
                                                                     nextL ? nextL->input_norm->getWeight()->data() : nullptr, T, (int)D, L.layer_scalar, cfg_.rms_norm_eps, st ) );
            return q8_next;
        }

        // ---- two halves of a chunk on two streams -------------------------------------------------------------------------------------------
        // A GEMM launch leaves CUs idle in its last round of tiles (fc_gate_up: 960 tiles on 256 CUs) and at every kernel boundary.  Rows are independent
        // but for attention, so the chunk's two halves run as two kernel sequences on two streams -- each on its own rows of every buffer -- and the second
        // half's attention of a layer waits (an event) for the first half's K / V rows of that layer.  The idle CUs of one stream's tails take the other
        // stream's workgroups.  Same kernels on the same rows: bit-identical to the one-stream form.
        // Not where any Linear of the chunk takes something from the context scratch -- staging, per-token activation rows (the fp8 x fp8 paths), a split-K workspace
        // (short tile lists: the same idle CUs this form is after): the two halves' calls would share it.  A split also depends on the row count, so the whole chunk's
        // row count is asked beside the half's: the halves carry the whole chunk's bits.  An op that stages per forward counts as taking scratch whatever these two
        // row counts need (usesContextScratch), so the form serves unquantized weights and the fp8 policy's resident bf16 copies, and never the fp4 policy, W8A8 or
        // per-forward staging.  (The FP8 KV cache dequantizes its band into the same scratch: setPrefillOverlap() refuses it.)
        bool overlapApplicable( dim_t T ) const
        {
            if ( !( T >= 1024 && T % 512 == 0 ) ) return false;
            for ( auto& L : layers_ )
                for ( int rows : { static_cast<int>( T ), static_cast<int>( T / 2 ) } )
                    if ( L.qkv_proj->getOperation().usesContextScratch( rows ) || L.o_proj->getOperation().usesContextScratch( rows ) ||
                         L.fc_gate_up->getOperation().gegluUsesContextScratch( rows ) || L.fc_down->getOperation().usesContextScratch( rows ) )
                        return false;
            return true;
        }
        TensorType* prefillOverlapped( const TokenTensor& tokens, dim_t T, dim_t position_offset )
        {
            const dim_t D = cfg_.embedding_dim;
            const int H = static_cast<int>( T / 2 );
            const auto dev = ctx_->getDeviceId();
            if ( !ov_qkv_ )
            {
                ov_qkv_ = std::make_unique<TensorType>( dev, shape_t{ 1, max_prefill_, std::max( cfg_.packedQkvWidth( false ), cfg_.packedQkvWidth( true ) ) } );
                ov_o_ = std::make_unique<TensorType>( dev, shape_t{ 1, max_prefill_, D } );
                ov_gate_up_ = std::make_unique<TensorType>( dev, shape_t{ 1, max_prefill_, 2 * cfg_.hidden_dim } );
                hipCheck( hipStreamCreateWithFlags( &ov_stream_, hipStreamNonBlocking ), "hipStreamCreate" );
                for ( auto& e : ov_ev_ ) hipCheck( hipEventCreateWithFlags( &e, hipEventDisableTiming ), "hipEventCreate" );
            }
            hipStream_t main = reinterpret_cast<hipStream_t>( ctx_->getStream() );
            embed( tokens.data(), static_cast<int>( T ), *pf_x_[ 0 ] );
            {
                // the first block's input norm over the whole chunk, before the streams part (the op's rstd rows are per call)
                auto x_all = pf_x_[ 0 ]->view( shape_t{ 1, T, D } );
                auto n_all = pf_norm_->view( shape_t{ 1, T, D } );
                layers_[ 0 ].input_norm->getOperation().forward( x_all, n_all );
            }
            hipCheck( hipEventRecord( ov_ev_[ 0 ], main ), "hipEventRecord" );
            hipCheck( hipStreamWaitEvent( ov_stream_, ov_ev_[ 0 ], 0 ), "hipStreamWaitEvent" );
            int flip = 0;
            for ( size_t i = 0; i < layers_.size(); ++i )
            {
                Layer* nextL = i + 1 < layers_.size() ? &layers_[ i + 1 ] : nullptr;
                hipEvent_t kv = ov_ev_[ 1 + ( i % 6 ) ];
                // each half's Linears write the two-stream form's own buffers (o is dead after the first tail: fc_down's rows go there too)
                BlockRows r{ 0, H, pf_x_[ flip ].get(), pf_x_[ 1 - flip ].get(), pf_norm_.get(), ov_qkv_.get(), ov_o_.get(), ov_gate_up_.get(), ov_o_.get(), false, kv, nullptr };
                blockPrefillFused( layers_[ i ], nextL, r, static_cast<int>( position_offset ) );
                {
                    struct Scope { Compute::RocmExecutionContext* c; mila_stream_t old; ~Scope() { c->swapStream( old ); } } scope{ ctx_, ctx_->swapStream( reinterpret_cast<mila_stream_t>( ov_stream_ ) ) };
                    r.row0 = H; r.kv_record = nullptr; r.kv_wait = kv;
                    blockPrefillFused( layers_[ i ], nextL, r, static_cast<int>( position_offset ) );
                }
                flip = 1 - flip;
            }
            hipCheck( hipEventRecord( ov_ev_[ 7 ], ov_stream_ ), "hipEventRecord" );
            hipCheck( hipStreamWaitEvent( main, ov_ev_[ 7 ], 0 ), "hipStreamWaitEvent" );
            return pf_x_[ flip ].get();
        }

    public:
        /// two half-chunks on two streams (see prefillOverlapped): off by default until measured per deployment; same bits either way
        void setPrefillOverlap( bool on )
        {
            if ( on && cfg_.kv_fp8 )
                throw std::invalid_argument( "GemmaTransformer::setPrefillOverlap: not available with kv_fp8 (both halves would dequantize their band into the one context scratch)" );
            prefill_overlap_ = on;
        }
        /// the fused prefill glue serves 1024 < D <= 8192 (workgroup-per-row canonical RMS reduction)
        bool fusedPrefillApplicable() const { return cfg_.embedding_dim > 1024 && cfg_.embedding_dim <= 8192 && cfg_.embedding_dim % 8 == 0; }
        /// on (default): prefill runs the fused glue when the configuration fits; off: one launch per reference op.  Same bits.
        void setFusedPrefill( bool on ) { fused_prefill_ = on; }
        /// fp4 policy: W4A8 prefill (fp4 -> e4m3 weights, per-token e4m3 activations, fp8 MFMA; the reference's default) on every
        /// layer Linear, or the exact-weight fallback (dequantize -> bf16 MFMA).
        /// fp8 policy: W8A8 prefill (the policy's e4m3 weights + per-channel scales on the fp8 matrix cores, no resident bf16 copy; default off -- the reference's
        /// arithmetic for this policy is W8A16) on every layer Linear.  No effect on unquantized weights.
        void setFp8ActivationPrefill( bool on )
        {
            if constexpr ( kFmt != 0 )
                for ( auto& L : layers_ )
                {
                    L.qkv_proj->getOperation().setFp8ActivationPrefill( on ); L.o_proj->getOperation().setFp8ActivationPrefill( on );
                    L.fc_gate_up->getOperation().setFp8ActivationPrefill( on ); L.fc_down->getOperation().setFp8ActivationPrefill( on );
                }
        }

    private:
        // ---- fused step ---------------------------------------------------------------------------------
        mila_fused_matvec_args baseArgs( LinearType& lin, uint16_t* y, const uint16_t* x ) const
        {
            mila_fused_matvec_args a{};
            a.y = y; a.x = x; a.W = lin.getWeight().rawData();
            a.scales = nullptr;
            if constexpr ( TWeightQuant::kIsQuantized ) a.scales = lin.getWeightScale()->data();
            a.post_scale = 1.0f; a.eps = cfg_.rms_norm_eps; a.fmt = kFmt; a.K = (int)lin.getConfig().getInputFeatures();
            a.N = (int)lin.getConfig().getOutputFeatures(); a.group = Quant::Weight::groupSizeOf<TWeightQuant>(); a.geglu = 0;
            return a;
        }
        // The three fused argument blocks of a decode step, for the one-row step and the rows step alike (the rows step adds its row strides: rowsArgs).
        /// [sandwich tail of the previous layer: post_ffn_norm, residual, layer scalar] + input_norm + qkv projection
        mila_fused_matvec_args qkvArgs( Layer& L, const Layer* prev, uint16_t* y, const uint16_t* x, const uint16_t* res, uint16_t* res_out ) const
        {
            auto a = baseArgs( *L.qkv_proj, y, x );
            a.norm_w = L.input_norm->getWeight()->data();
            if ( prev ) { a.post_w = prev->post_ffn_norm->getWeight()->data(); a.res = res; a.res_out = res_out; a.post_scale = prev->layer_scalar; }
            return a;
        }
        /// post_attn_norm + residual + pre_ffn_norm + gate_up + GeGLU
        mila_fused_matvec_args gateUpArgs( Layer& L, uint16_t* y, const uint16_t* x, const uint16_t* res, uint16_t* res_out ) const
        {
            auto a = baseArgs( *L.fc_gate_up, y, x );
            a.N = (int)cfg_.hidden_dim; a.geglu = 1;
            a.norm_w = L.pre_ffn_norm->getWeight()->data(); a.post_w = L.post_attn_norm->getWeight()->data();
            a.res = res; a.res_out = res_out;
            return a;
        }
        /// tail of the last layer + final norm + lm_head (fp32 logits); sampler_partials != nullptr: with the greedy sampler's first stage into `scratch`
        template <typename TScratch>
        mila_fused_matvec_args headArgs( const Layer& last, float* logits, const uint16_t* x, const uint16_t* res, uint16_t* res_out, TScratch& scratch, int* sampler_partials ) const
        {
            mila_fused_matvec_args a{};
            a.y = reinterpret_cast<uint16_t*>( logits ); a.x = x; a.W = lm_head_->getWeight().rawData();
            a.scales = nullptr;
            if constexpr ( kTableFmt != 0 ) a.scales = lm_head_->getWeightScale()->data();
            a.norm_w = final_norm_->getWeight()->data(); a.post_w = last.post_ffn_norm->getWeight()->data();
            a.res = res; a.res_out = res_out; a.post_scale = last.layer_scalar; a.eps = cfg_.rms_norm_eps;
            a.fmt = kTableFmt; a.K = (int)cfg_.embedding_dim; a.N = (int)cfg_.vocab_size; a.group = 0; a.geglu = 0; a.f32_out = 1;
            if ( sampler_partials ) { a.argmax_scratch = scratch.data(); a.argmax_scratch_bytes = scratch.sizeInBytes(); a.argmax_blocks = sampler_partials; }
            return a;
        }
        void fusedGateUp( Layer& L )
        {
            auto a = gateUpArgs( L, f_act_->data(), f_o_->data(), cur_hidden_, res1_->data() );
            Compute::rocmCheck( mila_cdna4_fused_norm_matvec( &a, ctx_->getStream() ) );
        }

        /// x_l (hidden) -> x_{l+1}.  The sandwich tail of layer l-1 (post_ffn_norm, residual, layer scalar)
        /// is the prologue of layer l's qkv kernel; the tail of the last layer is the prologue of the head.
        /// sampler_partials != nullptr: the head also runs the greedy sampler's first stage into sample_scratch_ and reports the number of partials
        void enqueueFusedStep( const int32_t* token_dev, int position, const int32_t* pos_dev, int* sampler_partials = nullptr )
        {
            mila_stream_t st = ctx_->getStream();
            embed( token_dev, 1, *hidden_[ 0 ] );
            cur_hidden_ = hidden_[ 0 ]->data();
            int next = 1;
            const Layer* prev = nullptr;
            for ( auto& L : layers_ )
            {
                const bool g = L.global;
                const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.numKvHeads( g ), HD = (int)cfg_.headDim( g );
                // 1. [tail of previous layer] + input_norm + qkv projection
                auto a = qkvArgs( L, prev, f_qkv_->data(), prev ? f_down_->data() : cur_hidden_, res1_->data(), hidden_[ next ]->data() );
                Compute::rocmCheck( mila_cdna4_fused_norm_matvec( &a, st ) );
                if ( prev ) { cur_hidden_ = hidden_[ next ]->data(); next = ( next == 1 ) ? 2 : 1; }
                // 2+3. q/k/v norms + RoPE + KV append + flash-decode in one launch (+ combine).
                //        qkv row = [q | k | v] (global: [q | k], V from the raw k projection)
                const uint16_t* qp = f_qkv_->data();
                const uint16_t* kp = qp + (size_t)NH * HD;
                const uint16_t* vp = g ? kp : kp + (size_t)NKV * HD;
                const size_t need = attnScratchBytes();
                void* scratch = attn_partials_->data();
                if ( L.kvFp8() )
                {
                    // the FP8 KV cache: two launches (+ combine) -- the quantizing append into a model-owned q buffer, then the policy's decode attention on the
                    // model-owned partials.  Under pos_dev, `position` is the live-length bound of the captured band bucket (as for the bf16 launch below)
                    const uint16_t *qw = L.q_norm->getWeight()->data(), *kw = L.k_norm->getWeight()->data(), *vw = L.v_norm->getWeight()->data();
                    const int cap = (int)L.cacheCapacity(), window = (int)cfg_.windowFor( g );
                    if ( pos_dev )
                    {
                        Compute::rocmCheck( mila_cdna4_fused_qkv_post_kvfp8_devpos( f_q_->data(), L.keyCacheFp8(), L.valueCacheFp8(), L.keyScales(), L.valueScales(), qp, kp, vp, qw, kw, vw,
                                                                                    L.rope->cosCache(), L.rope->sinCache(), NH, NKV, HD, pos_dev, cap, cfg_.rms_norm_eps, st ) );
                        Compute::rocmCheck( mila_cdna4_attn_decode_kvfp8_devpos( attn_out_->data(), f_q_->data(), L.keyCacheFp8(), L.valueCacheFp8(), L.keyScales(), L.valueScales(), scratch,
                                                                                 need, 1, NH, NKV, HD, cap, pos_dev, position, window, L.attentionScale(), st ) );
                    }
                    else
                    {
                        Compute::rocmCheck( mila_cdna4_fused_qkv_post_kvfp8( f_q_->data(), L.keyCacheFp8(), L.valueCacheFp8(), L.keyScales(), L.valueScales(), qp, kp, vp, qw, kw, vw,
                                                                             L.rope->cosCache(), L.rope->sinCache(), NH, NKV, HD, position, cap, cfg_.rms_norm_eps, st ) );
                        Compute::rocmCheck( mila_cdna4_attn_decode_kvfp8( attn_out_->data(), f_q_->data(), L.keyCacheFp8(), L.valueCacheFp8(), L.keyScales(), L.valueScales(), scratch, need,
                                                                          1, NH, NKV, HD, cap, position + 1, window, L.attentionScale(), st ) );
                    }
                }
                else
                    Compute::rocmCheck( mila_cdna4_fused_attn_decode_bf16( attn_out_->data(), L.keyCache(), L.valueCache(), qp, kp, vp, L.q_norm->getWeight()->data(),
                                                                           L.k_norm->getWeight()->data(), L.v_norm->getWeight()->data(), L.rope->cosCache(), L.rope->sinCache(),
                                                                           scratch, need, NH, NKV, HD, (int)L.cacheCapacity(), position, pos_dev,
                                                                           (int)cfg_.windowFor( g ), L.attentionScale(), cfg_.rms_norm_eps, st ) );
                // 4. o_proj
                L.o_proj->getOperation().matvec( f_o_->data(), attn_out_->data() );      // (the C-ABI call of Linear::forward on one row; these Linears carry no bias)
                // 5. post_attn_norm + residual + pre_ffn_norm + gate_up + GeGLU
                fusedGateUp( L );
                // 6. fc_down
                L.fc_down->getOperation().matvec( f_down_->data(), f_act_->data() );
                prev = &L;
            }
            // tail of the last layer + final norm + lm_head (fp32 logits) in one launch
            auto a = headArgs( *prev, logits_->data(), f_down_->data(), res1_->data(), hidden_[ next ]->data(), *sample_scratch_, sampler_partials );
            Compute::rocmCheck( mila_cdna4_fused_norm_matvec( &a, st ) );
        }


        // ---- rows step ------------------------------------------------------------------------------------
        mila_matvec_rows_args rowsArgs( const mila_fused_matvec_args& a, int B, dim_t x_stride, dim_t y_stride, dim_t res_stride = 0, dim_t res_out_stride = 0 ) const
        {
            mila_matvec_rows_args r{};
            r.a = a; r.bias = nullptr; r.rows = B;
            r.x_stride = x_stride; r.y_stride = y_stride; r.res_stride = res_stride; r.res_out_stride = res_out_stride;
            return r;
        }
        /// where a chain step's rows sit: row t at position + t (eager), or at *pos_dev + t (the one-row graph's position word)
        struct ChainAt { int position; const int32_t* pos_dev; };
        /// enqueueFusedStep for rows 0 .. B - 1: the same launches on the rows entries.  max_len: the live-length bound of the captured band bucket.
        /// chain != nullptr: the rows are consecutive positions of the ONE sequence on the one cache -- the chain attention entry in place of the rows one
        void enqueueFusedStepRows( int B, int max_len, int* sampler_partials, const ChainAt* chain = nullptr )
        {
            mila_stream_t st = ctx_->getStream();
            auto& R = *rows_;
            const dim_t D = cfg_.embedding_dim, F = cfg_.hidden_dim, PK = std::max( cfg_.packedQkvWidth( false ), cfg_.packedQkvWidth( true ) );
            embed( R.tok->data(), B, *R.hidden[ 0 ] );
            const uint16_t* cur = R.hidden[ 0 ]->data();
            int next = 1;
            const Layer* prev = nullptr;
            for ( auto& L : layers_ )
            {
                const bool g = L.global;
                const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.numKvHeads( g ), HD = (int)cfg_.headDim( g );
                // 1. [tail of previous layer] + input_norm + qkv projection; the rows of the packed projection are PK elements apart
                auto a = qkvArgs( L, prev, R.qkv->data(), prev ? R.down->data() : cur, R.res1->data(), R.hidden[ next ]->data() );
                auto r = rowsArgs( a, B, D, PK, D, D );
                Compute::rocmCheck( mila_cdna4_matvec_rows( &r, st ) );
                if ( prev ) { cur = R.hidden[ next ]->data(); next = ( next == 1 ) ? 2 : 1; }
                // 2+3. q/k/v norms + RoPE + KV append + flash-decode, row b at pos[ b ] on its own caches (+ combine); output rows NH * HD apart
                const uint16_t* qp = R.qkv->data();
                const uint16_t* kp = qp + (size_t)NH * HD;
                const uint16_t* vp = g ? kp : kp + (size_t)NKV * HD;
                if ( chain )
                    Compute::rocmCheck( mila_cdna4_fused_attn_chain_bf16( R.attn->data(), L.keyCache(), L.valueCache(), qp, kp, vp, (int64_t)PK, L.q_norm->getWeight()->data(),
                                                                                 L.k_norm->getWeight()->data(), L.v_norm->getWeight()->data(), L.rope->cosCache(), L.rope->sinCache(),
                                                                                 R.attn_partials->data(), R.attn_partials->sizeInBytes(), B, NH, NKV, HD, (int)L.cacheCapacity(),
                                                                                 chain->position, chain->pos_dev, max_len, (int)cfg_.windowFor( g ), L.attentionScale(),
                                                                                 cfg_.rms_norm_eps, st ) );
                else if ( L.kvFp8() )
                {
                    // the FP8 KV cache: two launches (+ combine), as in the one-row step -- the quantizing append of every row into its own caches and the rows q
                    // buffer, then the policy's decode attention, row b over pos[ b ] + 1 keys, on the rows partials
                    const int cap = (int)L.cacheCapacity();
                    Compute::rocmCheck( mila_cdna4_fused_qkv_post_kvfp8_rows_devpos( R.q->data(), L.keyCacheFp8Rows(), L.valueCacheFp8Rows(), L.keyScalesRows(), L.valueScalesRows(), qp, kp, vp,
                                                                                     (int64_t)PK, L.q_norm->getWeight()->data(), L.k_norm->getWeight()->data(), L.v_norm->getWeight()->data(),
                                                                                     L.rope->cosCache(), L.rope->sinCache(), B, NH, NKV, HD, R.pos->data(), cap, cfg_.rms_norm_eps, st ) );
                    Compute::rocmCheck( mila_cdna4_attn_decode_kvfp8_rows( R.attn->data(), R.q->data(), L.keyCacheFp8Rows(), L.valueCacheFp8Rows(), L.keyScalesRows(), L.valueScalesRows(),
                                                                           R.attn_partials->data(), R.attn_partials->sizeInBytes(), B, NH, NKV, HD, cap, R.pos->data(), max_len,
                                                                           (int)cfg_.windowFor( g ), L.attentionScale(), st ) );
                }
                else
                    Compute::rocmCheck( mila_cdna4_fused_attn_decode_rows_bf16( R.attn->data(), L.keyCacheRows(), L.valueCacheRows(), qp, kp, vp, (int64_t)PK, L.q_norm->getWeight()->data(),
                                                                                L.k_norm->getWeight()->data(), L.v_norm->getWeight()->data(), L.rope->cosCache(), L.rope->sinCache(),
                                                                                R.attn_partials->data(), R.attn_partials->sizeInBytes(), B, NH, NKV, HD, (int)L.cacheCapacity(), R.pos->data(),
                                                                                ringRows() && !g ? std::min( max_len, (int)L.cacheCapacity() ) : max_len, (int)cfg_.windowFor( g ),
                                                                                L.attentionScale(), cfg_.rms_norm_eps, st ) );      // (a ring layer: the entry wants max_len <= capacity, and its plan is the window's anyway)
                // 4. o_proj
                L.o_proj->getOperation().matvecRows( R.o->data(), R.attn->data(), B, (int64_t)NH * HD, D );
                // 5. post_attn_norm + residual + pre_ffn_norm + gate_up + GeGLU
                a = gateUpArgs( L, R.act->data(), R.o->data(), cur, R.res1->data() );
                r = rowsArgs( a, B, D, F, D, D );
                Compute::rocmCheck( mila_cdna4_matvec_rows( &r, st ) );
                // 6. fc_down
                L.fc_down->getOperation().matvecRows( R.down->data(), R.act->data(), B, F, D );
                prev = &L;
            }
            // tail of the last layer + final norm + lm_head (fp32 logits, one set of sampler partials per row) in one launch
            auto a = headArgs( *prev, R.logits->data(), R.down->data(), R.res1->data(), R.hidden[ next ]->data(), *R.sample_scratch, sampler_partials );
            auto r = rowsArgs( a, B, D, cfg_.vocab_size, D, D );
            Compute::rocmCheck( mila_cdna4_matvec_rows( &r, st ) );
        }
        void enqueueRowsStepAndTail( int B, dim_t band, bool greedy )
        {
            int partials = 0;
            if ( !row_requests_.empty() ) { enqueueRowsRequestsStepAndTail( B, band ); return; }
            if ( step_lp_ && !greedy && !rowsSamplesInStep() )
                throw std::invalid_argument( "GemmaTransformer: token log-probabilities need a sampler tail in the rows step (greedy, or setRowsSampling)" );
            if ( automaton_on_ ) throw std::invalid_argument( "GemmaTransformer: the rows step takes no token automaton: one state per row is not built (clearTokenAutomaton)" );
            const bool penalized_greedy = greedy && ( filters_.penalized() || bias_on_ );      // the lm_head epilogue cannot compute the adjusted logits: the step ends at the logits
            enqueueFusedStepRows( B, static_cast<int>( band ), ( greedy && !penalized_greedy ) ? &partials : nullptr );
            auto& R = *rows_;
            if ( !greedy && rowsSamplesInStep() && ( rows_sampling_->filtered() || bias_on_ ) )      // (one bias table for every row: stride 0)
            {
                const mila_sample_filters f = rows_sampling_->filters();
                Compute::rocmCheck( mila_cdna4_sample_radix_biased_rows_advance_fp32( R.logits->data(), static_cast<size_t>( cfg_.vocab_size ), R.tok->data(), B, (int)cfg_.vocab_size,
                                                                                      cfg_.final_logit_softcapping, rows_sampling_->temperature, rows_sampling_->top_k,
                                                                                      rows_sampling_->top_p, rows_draws_, &f, tableWords( *rows_sampling_, 0, false ),
                                                                                      static_cast<size_t>( cfg_.vocab_size ), biasValues(), 0, R.radix_scratch->data(),
                                                                                      R.radix_scratch->sizeInBytes(), R.pos->data(), R.active->data(), ctx_->getStream() ) );
            }
            else if ( penalized_greedy )
            {
                const mila_sample_filters f = filters_.filters();
                Compute::rocmCheck( mila_cdna4_sample_argmax_biased_rows_advance_fp32( R.logits->data(), static_cast<size_t>( cfg_.vocab_size ), R.tok->data(), B, (int)cfg_.vocab_size,
                                                                                       cfg_.final_logit_softcapping, &f, tableWords( filters_, 0, false ),
                                                                                       static_cast<size_t>( cfg_.vocab_size ), biasValues(), 0, R.sample_scratch->data(),
                                                                                       R.sample_scratch->sizeInBytes(), R.pos->data(), R.active->data(), ctx_->getStream() ) );
            }
            else if ( !greedy && rowsSamplesInStep() )      // the radix pipeline over the B rows behind the logits; its tail takes the place of the position bump
                Compute::rocmCheck( mila_cdna4_sample_radix_rows_advance_fp32( R.logits->data(), static_cast<size_t>( cfg_.vocab_size ), R.tok->data(), B, (int)cfg_.vocab_size,
                                                                               cfg_.final_logit_softcapping, rows_sampling_->temperature, rows_sampling_->top_k, rows_sampling_->top_p,
                                                                               rows_draws_, R.radix_scratch->data(), R.radix_scratch->sizeInBytes(), R.pos->data(), R.active->data(),
                                                                               ctx_->getStream() ) );
            else if ( greedy )
                Compute::rocmCheck( mila_cdna4_sample_argmax_rows_final_advance( R.tok->data(), R.sample_scratch->data(), R.sample_scratch->sizeInBytes(), partials, R.pos->data(),
                                                                                 R.active->data(), B, ctx_->getStream() ) );
            else
                Compute::rocmCheck( mila_cdna4_advance_positions_rows( R.pos->data(), R.active->data(), B, ctx_->getStream() ) );
            // the tail wrote the active rows' tokens: their log-probabilities; an inactive row's outputs stay as they are
            if ( step_lp_ ) lp_op_->forward( R.logits->data(), static_cast<size_t>( cfg_.vocab_size ), R.tok->data(), B, step_lp_->top_n, R.active->data(), nullptr );
        }
        /// The rows step of row requests (setRowsRequests): the layers, then the stochastic rows' radix pipeline and the greedy rows' argmax pair, each reading its row's
        /// record -- the two tails together advance every active row exactly once -- then the automaton rows step and the log-probability launches.  A batch without
        /// greedy (stochastic) rows holds no argmax (radix) launches.  One linear chain on one stream.
        void enqueueRowsRequestsStepAndTail( int B, dim_t band )
        {
            const RowsRequestKey k = rowsRequestKey();
            if ( k.stochastic && !row_request_draws_ ) throw std::invalid_argument( "GemmaTransformer: a stochastic row request needs the rows' draws (setRowsRequests)" );
            if ( k.table && !token_table_ ) throw std::logic_error( "GemmaTransformer: penalties without a token table (setRowsRequests allocates it)" );
            enqueueFusedStepRows( B, static_cast<int>( band ), nullptr );
            auto& R = *rows_;
            const size_t V = static_cast<size_t>( cfg_.vocab_size );
            uint32_t* table = k.table ? token_table_->data() : nullptr;
            const float* bias = k.constrained ? row_bias_->eff() : nullptr;
            if ( k.stochastic )
                Compute::rocmCheck( mila_cdna4_sample_radix_requests_rows_advance_fp32( R.logits->data(), V, R.tok->data(), B, (int)cfg_.vocab_size, cfg_.final_logit_softcapping,
                                                                                        row_params_->rawData(), row_request_draws_, table, V, bias, V, R.radix_scratch->data(),
                                                                                        R.radix_scratch->sizeInBytes(), R.pos->data(), R.active->data(), ctx_->getStream() ) );
            // (a stochastic row's zero table adds +0.0 in front of a value whose sign of zero the scale launch canonicalizes anyway: one radix call serves both kinds)
            if ( k.greedy_constrained )
                Compute::rocmCheck( mila_cdna4_sample_argmax_requests_rows_advance_fp32( R.logits->data(), V, R.tok->data(), B, (int)cfg_.vocab_size, cfg_.final_logit_softcapping,
                                                                                         row_params_->rawData(), table, V, bias, V, R.sample_scratch->data(),
                                                                                         R.sample_scratch->sizeInBytes(), R.pos->data(), row_masks_->data(), ctx_->getStream() ) );
            if ( k.greedy_plain )
                Compute::rocmCheck( mila_cdna4_sample_argmax_requests_rows_advance_fp32( R.logits->data(), V, R.tok->data(), B, (int)cfg_.vocab_size, cfg_.final_logit_softcapping,
                                                                                         row_params_->rawData(), table, V, nullptr, 0, R.sample_scratch->data(),
                                                                                         R.sample_scratch->sizeInBytes(), R.pos->data(), row_masks_->data() + cfg_.max_batch,
                                                                                         ctx_->getStream() ) );
            if ( k.automaton ) row_automata_->step( *row_bias_, R.tok->data(), R.active->data(), B );
            if ( step_lp_ ) lp_op_->forward( R.logits->data(), V, R.tok->data(), B, step_lp_->top_n, R.active->data(), nullptr );
        }
        /// a chain step and its tail: the rows step on the chain attention entry, then the accept kernel on the ONE position word (tok[ 0 ] <- the last accepted
        /// token, result <- {count, accepted tokens}, position += count).  One linear chain on one stream.
        void enqueueChainStepAndTail( int T, dim_t band, const ChainAt& at )
        {
            int partials = 0;
            if ( filters_.penalized() ) throw std::invalid_argument( "GemmaTransformer: the chain step takes no penalties (setSamplingFilters)" );
            const bool stochastic = chainSamples(), constrained = bias_on_ || automaton_on_;
            auto& R = *rows_;
            // the constrained chain step (mila_cdna4.h): row t's table is row t of the automaton's effective table, composed here for the state behind the drafts
            // 1 .. t (row 0 holds the table of the state word from the step before), or the ONE bias table for every row (stride 0)
            if ( automaton_on_ ) token_automaton_->chainCompose( biasValues(), R.tok->data(), T );
            const float* tables = samplerBias();
            const size_t tables_stride = automaton_on_ ? static_cast<size_t>( cfg_.vocab_size ) : 0;
            enqueueFusedStepRows( T, static_cast<int>( band ), stochastic || constrained ? nullptr : &partials, &at );      // stochastic / constrained: the lm_head leaves the logits only
            if ( stochastic && constrained )
                Compute::rocmCheck( mila_cdna4_sample_radix_biased_chain_accept_fp32( R.tok->data(), R.result->data(), R.logits->data(), static_cast<size_t>( cfg_.vocab_size ), T,
                                                                                      (int)cfg_.vocab_size, cfg_.final_logit_softcapping, chain_sampling_->temperature,
                                                                                      chain_sampling_->top_k, chain_sampling_->top_p, chain_draws_, tables, tables_stride,
                                                                                      R.radix_scratch->data(), R.radix_scratch->sizeInBytes(), pos_dev_->data(), ctx_->getStream() ) );
            else if ( constrained )
                Compute::rocmCheck( mila_cdna4_sample_argmax_biased_chain_accept_fp32( R.tok->data(), R.result->data(), R.logits->data(), static_cast<size_t>( cfg_.vocab_size ), T,
                                                                                       (int)cfg_.vocab_size, cfg_.final_logit_softcapping, tables, tables_stride,
                                                                                       R.sample_scratch->data(), R.sample_scratch->sizeInBytes(), pos_dev_->data(), ctx_->getStream() ) );
            else if ( stochastic )
                Compute::rocmCheck( mila_cdna4_sample_radix_chain_accept_fp32( R.tok->data(), R.result->data(), R.logits->data(), static_cast<size_t>( cfg_.vocab_size ), T,
                                                                               (int)cfg_.vocab_size, cfg_.final_logit_softcapping, chain_sampling_->temperature, chain_sampling_->top_k,
                                                                               chain_sampling_->top_p, chain_draws_, R.radix_scratch->data(), R.radix_scratch->sizeInBytes(),
                                                                               pos_dev_->data(), ctx_->getStream() ) );
            else
                Compute::rocmCheck( mila_cdna4_sample_argmax_chain_accept( R.tok->data(), R.result->data(), R.sample_scratch->data(), R.sample_scratch->sizeInBytes(), partials, pos_dev_->data(), T,
                                                                       ctx_->getStream() ) );
            if ( automaton_on_ ) token_automaton_->chainStep( biasValues(), R.tok->data(), R.result->data(), T );      // the state word and row 0 for the next step, of either kind
            // result = {count, accepted tokens}: row t < count reports result[ 1 + t ] under row t's logits; the rejected rows have no token
            if ( step_lp_ ) lp_op_->forward( R.logits->data(), static_cast<size_t>( cfg_.vocab_size ), R.result->data() + 1, T, step_lp_->top_n, nullptr, R.result->data() );
        }
        bool rowsSamplesInStep() const noexcept { return rows_sampling_.has_value() && rows_draws_ != nullptr; }
        bool chainSamples() const noexcept { return chain_sampling_.has_value() && chain_draws_ != nullptr; }
        void requireChain() const
        {
            if ( !rows_ || cfg_.draft_tokens <= 0 ) throw std::logic_error( "GemmaTransformer: the chain interface needs GemmaConfig::draft_tokens > 0" );
        }
        void checkChainStep( int T, dim_t position ) const
        {
            requireChain();
            if ( T < 2 || T > cfg_.draft_tokens + 1 )
                throw std::invalid_argument( "GemmaTransformer: a chain step takes 2 .. draft_tokens + 1 rows (got " + std::to_string( T ) + ")" );
            checkPosition( position, T );
            if ( bandBucket( position ) != bandBucket( position + T - 1 ) )
                throw std::invalid_argument( "GemmaTransformer: a chain step must not cross a live-length bucket (positions " + std::to_string( position ) + " .. " +
                                             std::to_string( position + T - 1 ) + "): its later rows would not have the bits they have alone" );
        }
        void destroyGraphChain()
        {
            if ( chain_graph_exec_ ) { (void)hipGraphExecDestroy( chain_graph_exec_ ); chain_graph_exec_ = nullptr; }
            if ( chain_graph_ ) { (void)hipGraphDestroy( chain_graph_ ); chain_graph_ = nullptr; }
        }
        /// every layer's cache prefix in one launch, from the table buildRows() made (mila_cdna4.h: kv_rows_fork_layers_bf16, kv_rows_fork_layers_kvfp8)
        void forkLayers( int src, unsigned dst_mask, dim_t len )
        {
            if ( !fork_layers_fp8_.empty() )
            {
                Compute::rocmCheck( mila_cdna4_kv_rows_fork_layers_kvfp8( fork_layers_fp8_.data(), static_cast<int>( fork_layers_fp8_.size() ), static_cast<int>( cfg_.max_batch ), src,
                                                                          dst_mask, static_cast<int>( len ), ctx_->getStream() ) );
                return;
            }
            if ( !fork_layers_band_.empty() )      // a ring model: every layer's live band, and what the destination rows hold from now on
            {
                Compute::rocmCheck( mila_cdna4_kv_rows_fork_layers_band_bf16( fork_layers_band_.data(), static_cast<int>( fork_layers_band_.size() ), static_cast<int>( cfg_.max_batch ), src,
                                                                              dst_mask, static_cast<int>( len ), ctx_->getStream() ) );
                for ( size_t r = 0; r < row_high_.size(); ++r )
                    if ( ( dst_mask >> r ) & 1u ) { row_high_[ r ] = len; row_from_[ r ] = std::max<dim_t>( 0, len - cfg_.window + 1 ); }
                return;
            }
            Compute::rocmCheck( mila_cdna4_kv_rows_fork_layers_bf16( fork_layers_.data(), static_cast<int>( fork_layers_.size() ), static_cast<int>( cfg_.max_batch ), src, dst_mask,
                                                                     static_cast<int>( len ), ctx_->getStream() ) );
        }
        /// A ring model's account of row b (GemmaConfig::bounded_local_kv_rows; Mila/PrefixCache.h states the rule): row_high_ -- the furthest length written since the row
        /// was last written from position 0, as far as prefillRow / forkRow / forkRowPrefix / rewindKvCacheRow were told (steps advance on the device: their callers pass
        /// `written`); row_from_ -- the lowest position a band fork is known to have left intact.  Positions below max( row_from_, row_high_ - capacity + 1 ) count as gone.
        bool ringRows() const noexcept { return ring_capacity_ > 0; }
        dim_t rowValidFrom( int b ) const noexcept { return std::max<dim_t>( { 0, row_from_[ static_cast<size_t>( b ) ], row_high_[ static_cast<size_t>( b ) ] - ring_capacity_ + 1 } ); }
        bool rowHolds( int b, dim_t position ) const noexcept { return std::max<dim_t>( 0, position - cfg_.window + 1 ) >= rowValidFrom( b ); }      // PrefixCache::usable, on this account
        void requireRows( int b ) const
        {
            if ( !rows_ || cfg_.max_batch <= 1 ) throw std::logic_error( "GemmaTransformer: the rows interface needs GemmaConfig::max_batch > 1" );
            if ( b < 0 || b >= cfg_.max_batch ) throw std::invalid_argument( "GemmaTransformer: row " + std::to_string( b ) + " outside max_batch " + std::to_string( cfg_.max_batch ) );
        }
        void checkRowsStep( int B, dim_t max_position ) const
        {
            requireRows( 0 );
            if ( B < 2 || B > cfg_.max_batch ) throw std::invalid_argument( "GemmaTransformer: a rows step takes 2 .. max_batch rows (got " + std::to_string( B ) + ")" );
            checkPosition( max_position, 1 );
        }
        void setRowWord( int32_t* words, int b, int32_t v )
        {
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( words + b, &v, 4, ctx_->getStream() ) );
            ctx_->synchronize();
        }
        void destroyGraphRows()
        {
            if ( rows_graph_exec_ ) { (void)hipGraphExecDestroy( rows_graph_exec_ ); rows_graph_exec_ = nullptr; }
            if ( rows_graph_ ) { (void)hipGraphDestroy( rows_graph_ ); rows_graph_ = nullptr; }
        }
        /// the decode-role buffers of a rows step, [rows, width] each; allocated only when max_batch > 1 (rows = max_batch, with a KV cache per row) or draft_tokens > 0
        /// (rows = draft_tokens + 1 on the ONE cache, plus the chain's result words), so a model with neither is byte for byte what it was
        struct RowsState
        {
            std::unique_ptr<TensorType> qkv, attn, o, down, act, res1, hidden[ 3 ];
            std::unique_ptr<TensorType> q;      // FP8 KV rows only: [rows, NH * HD] roped q rows
            std::unique_ptr<LogitsTensor> logits, sample_scratch, attn_partials;
            std::unique_ptr<LogitsTensor> radix_scratch;      // the rows radix sampler's workspace, one region per row
            std::unique_ptr<TokenTensor> pos, tok, active;
            std::unique_ptr<TokenTensor> result;      // chain only: {count, accepted tokens ...}, draft_tokens + 2 words
        };
        dim_t rowsCount() const noexcept { return cfg_.max_batch > 1 ? cfg_.max_batch : cfg_.draft_tokens + 1; }
        void buildRows()
        {
            const dim_t B = rowsCount(), D = cfg_.embedding_dim;
            const auto dev = ctx_->getDeviceId();
            if ( cfg_.max_batch > 1 )
            {
                fork_layers_.clear();      // the layer tables of forkRow / forkRowPrefix (one per cache policy; a model has layers of one): built once, here
                fork_layers_fp8_.clear();
                fork_layers_band_.clear();
                ring_capacity_ = 0;
                row_high_.assign( static_cast<size_t>( B ), 0 );
                row_from_.assign( static_cast<size_t>( B ), 0 );
                for ( auto& L : layers_ )
                {
                    L.setCacheRows( static_cast<int>( B ) );
                    const auto NKV = static_cast<int32_t>( cfg_.numKvHeads( L.global ) ), cap = static_cast<int32_t>( L.cacheCapacity() ), HD = static_cast<int32_t>( cfg_.headDim( L.global ) );
                    if ( L.kvFp8() ) fork_layers_fp8_.push_back( mila_kv_fork_layer_fp8{ L.keyCacheFp8Rows(), L.valueCacheFp8Rows(), L.keyScalesRows(), L.valueScalesRows(), NKV, cap, HD, 0 } );
                    else if ( cfg_.bounded_local_kv_rows )      // rings on the sliding-window layers: the live band of each (a global layer: window 0, the whole prefix)
                    {
                        fork_layers_band_.push_back( mila_kv_fork_layer_band{ L.keyCacheRows(), L.valueCacheRows(), NKV, cap, HD, static_cast<int32_t>( cfg_.windowFor( L.global ) ) } );
                        if ( !L.global ) ring_capacity_ = cap;
                    }
                    else fork_layers_.push_back( mila_kv_fork_layer{ L.keyCacheRows(), L.valueCacheRows(), NKV, cap, HD, 0 } );
                }
            }
            rows_ = std::make_unique<RowsState>();
            auto& R = *rows_;
            // the FP8 rows step's roped q rows, between its two launches per layer (a bf16 rows model allocates none: byte for byte what it was)
            if ( cfg_.max_batch > 1 && cfg_.kv_fp8 ) R.q = std::make_unique<TensorType>( dev, shape_t{ B, std::max( cfg_.qWidth( false ), cfg_.qWidth( true ) ) } );
            R.qkv = std::make_unique<TensorType>( dev, shape_t{ B, std::max( cfg_.packedQkvWidth( false ), cfg_.packedQkvWidth( true ) ) } );
            R.attn = std::make_unique<TensorType>( dev, shape_t{ B, std::max( cfg_.qWidth( false ), cfg_.qWidth( true ) ) } );
            R.o = std::make_unique<TensorType>( dev, shape_t{ B, D } );
            R.down = std::make_unique<TensorType>( dev, shape_t{ B, D } );
            R.act = std::make_unique<TensorType>( dev, shape_t{ B, cfg_.hidden_dim } );
            R.res1 = std::make_unique<TensorType>( dev, shape_t{ B, D } );
            for ( auto& h : R.hidden ) h = std::make_unique<TensorType>( dev, shape_t{ B, 1, D } );
            R.logits = std::make_unique<LogitsTensor>( dev, shape_t{ B, 1, cfg_.vocab_size } );
            R.sample_scratch = std::make_unique<LogitsTensor>( dev, shape_t{ B, static_cast<dim_t>( mila_cdna4_sample_scratch_bytes() / 4 ) } );
            R.attn_partials = std::make_unique<LogitsTensor>( dev, shape_t{ static_cast<dim_t>( ( rowsAttnScratchBytes() + 3 ) / 4 ) } );
            R.radix_scratch = std::make_unique<LogitsTensor>( dev, shape_t{ static_cast<dim_t>( rowsRadixScratchBytes() / 4 ) } );
            R.pos = std::make_unique<TokenTensor>( dev, shape_t{ B } );
            R.tok = std::make_unique<TokenTensor>( dev, shape_t{ B } );
            R.active = std::make_unique<TokenTensor>( dev, shape_t{ B } );
            if ( cfg_.draft_tokens > 0 )
            {
                R.result = std::make_unique<TokenTensor>( dev, shape_t{ B + 1 } );
                Compute::rocmCheck( mila_cdna4_memset_zero( R.result->data(), R.result->sizeInBytes(), ctx_->getStream() ) );
            }
            // every row starts as a valid, inactive sequence at position 0 with token 0: a row that was never admitted still rides through a step's launches
            for ( auto* t : { R.pos.get(), R.tok.get(), R.active.get() } ) Compute::rocmCheck( mila_cdna4_memset_zero( t->data(), t->sizeInBytes(), ctx_->getStream() ) );
            for ( auto* t : { R.qkv.get(), R.attn.get(), R.o.get(), R.down.get(), R.act.get(), R.res1.get() } ) Compute::rocmCheck( mila_cdna4_memset_zero( t->data(), t->sizeInBytes(), ctx_->getStream() ) );
        }
        size_t rowsAttnScratchBytes() const
        {
            const int B = static_cast<int>( rowsCount() );
            if ( cfg_.draft_tokens > 0 )      // the chain entry parks the roped q rows behind the partials at every head size
                return std::max( mila_cdna4_attn_chain_scratch_bytes( B, (int)cfg_.num_heads, (int)cfg_.head_dim ),
                                 mila_cdna4_attn_chain_scratch_bytes( B, (int)cfg_.num_heads, (int)cfg_.global_head_dim ) );
            return std::max( mila_cdna4_attn_decode_scratch_bytes( B, (int)cfg_.num_heads, (int)cfg_.head_dim ), mila_cdna4_attn_decode_scratch_bytes( B, (int)cfg_.num_heads, (int)cfg_.global_head_dim ) );
        }
        /// the rows radix sampler's workspace for rowsCount() rows (a multiple of 8)
        size_t rowsRadixScratchBytes() const { return mila_cdna4_sample_radix_rows_scratch_bytes( static_cast<int>( rowsCount() ), (int)cfg_.vocab_size ); }
        size_t rowsStateBytes() const
        {
            if ( !rows_ ) return 0;
            size_t b = 0;
            auto& R = *rows_;
            for ( const auto* t : { R.qkv.get(), R.attn.get(), R.o.get(), R.down.get(), R.act.get(), R.res1.get(), R.hidden[ 0 ].get(), R.hidden[ 1 ].get(), R.hidden[ 2 ].get() } ) b += tensorBytes( t );
            for ( const auto* t : { R.logits.get(), R.sample_scratch.get(), R.attn_partials.get(), R.radix_scratch.get() } ) b += tensorBytes( t );
            for ( const auto* t : { R.pos.get(), R.tok.get(), R.active.get() } ) b += tensorBytes( t );
            if ( R.result ) b += tensorBytes( R.result.get() );
            if ( R.q ) b += tensorBytes( R.q.get() );
            return b;
        }
        /// the same from the configuration alone, plus the cache rows beyond the first of every layer
        size_t requiredRowsStateBytes() const
        {
            if ( cfg_.max_batch <= 1 && cfg_.draft_tokens <= 0 ) return 0;
            const size_t B = static_cast<size_t>( rowsCount() ), D = static_cast<size_t>( cfg_.embedding_dim );
            const size_t maxq = static_cast<size_t>( std::max( cfg_.qWidth( false ), cfg_.qWidth( true ) ) ), maxpacked = static_cast<size_t>( std::max( cfg_.packedQkvWidth( false ), cfg_.packedQkvWidth( true ) ) );
            size_t b = B * ( maxpacked + maxq + 3 * D + static_cast<size_t>( cfg_.hidden_dim ) + 3 * D ) * 2;
            b += B * static_cast<size_t>( cfg_.vocab_size ) * 4 + B * ( ( mila_cdna4_sample_scratch_bytes() / 4 ) * 4 ) + ( ( rowsAttnScratchBytes() + 3 ) / 4 ) * 4 + 3 * B * 4;
            b += rowsRadixScratchBytes();
            if ( cfg_.draft_tokens > 0 ) return b + ( B + 1 ) * 4;      // the chain's result words; its rows share the one cache
            if ( cfg_.kv_fp8 ) return b + B * maxq * 2;      // the rows q buffer; the FP8 KV op counts its cache rows itself (RocmGqaKvFp8Op::requiredStateBytes)
            for ( auto& L : layers_ ) b += ( B - 1 ) * 2 * static_cast<size_t>( cfg_.kvWidth( L.global ) ) * static_cast<size_t>( L.cacheCapacity() ) * 2;
            return b;
        }

    public:
        // ------------------------------------------------------------------------------------
        // weight ingestion.  Tensor vocabulary = the reference's flat names (the root's own name dropped,
        // Core/LanguageModel.ixx:137-146): `tf_layer_<i>.<child>.weight` (+ `.weight_scale` for a quantized Linear, Linear.ixx:370-400),
        // `tf_layer_<i>.layer_scalar` ([1] F32, Gemma.Block.ixx:546-560), `temb.wte` (+ `temb.wte_scale`, TokenEmbedding.ixx:351-384),
        // `rmsn_final.weight`; a tied model has NO `lm_head.weight` (Gemma.ixx:540-555) -- the head adopts the embedding table.
        // Readers accept the names with or without the `<model name>.` prefix (CompositeComponent::findComponent strips it).
        // ------------------------------------------------------------------------------------
        static const char* weightQuantizationName() { return kFmt == 0 ? "none" : kFmt == 1 ? "per_channel_fp8_e4m3" : "per_group_fp4_128"; }   // LanguageModelConfig.ixx:104-114

        Serialization::PretrainedMetadata pretrainedMetadata() const
        {
            Serialization::PretrainedMetadata m;
            m.architecture = "gemma4"; m.model_name = name_;
            m.vocab_size = (uint32_t)cfg_.vocab_size; m.max_seq_length = (uint32_t)max_seq_; m.embedding_dim = (uint32_t)cfg_.embedding_dim; m.num_layers = (uint32_t)cfg_.num_layers;
            m.num_heads = (uint32_t)cfg_.num_heads; m.num_kv_heads = (uint32_t)cfg_.num_kv_heads; m.head_dim = (uint32_t)cfg_.head_dim; m.hidden_dim = (uint32_t)cfg_.hidden_dim;
            m.use_bias = false; m.tie_word_embeddings = true; m.activation = "gelu"; m.norm_type = "rmsnorm"; m.attention_type = "gqa"; m.positional_encoding = "rope";
            m.rope_theta = cfg_.rope_theta_local; m.norm_epsilon = cfg_.rms_norm_eps;
            m.global_head_dim = (uint32_t)cfg_.global_head_dim; m.num_global_kv_heads = (uint32_t)cfg_.num_global_kv_heads; m.key_equals_value = true;
            m.window = (uint32_t)cfg_.window; m.sliding_window_pattern = (uint32_t)cfg_.sliding_window_pattern; m.global_rotary_dim = (uint32_t)cfg_.global_rotary_dim;
            m.rope_theta_local = cfg_.rope_theta_local; m.rope_theta_global = cfg_.rope_theta_global; m.final_logit_softcapping = cfg_.final_logit_softcapping;
            return m;
        }

    private:
        struct SaveItem { std::string name, dtype; std::vector<int64_t> shape; const void* dev; size_t bytes; float host_scalar; };
        /// the model's tensors in the reference's declaration order (block children in createGraph order, then the block's own scalar)
        std::vector<SaveItem> saveItems()
        {
            std::vector<SaveItem> items;
            auto shapeOf = []( const auto& t ) { std::vector<int64_t> v; for ( auto d : t.shape() ) v.push_back( (int64_t)d ); return v; };
            auto storageName = []( auto& lin )
            {
                using L = std::remove_reference_t<decltype( lin )>;
                if constexpr ( !L::kIsQuantized ) return "BF16"; else return L::kWeightDtype == TensorDataType::FP8_E4M3 ? "F8_E4M3" : "U8";
            };
            auto addLinear = [&]( auto& lin, const std::string& flat, const char* wname, const char* sname )
            {
                auto& w = lin.getWeight();
                items.push_back( { flat + "." + wname, storageName( lin ), shapeOf( w ), w.rawData(), w.sizeInBytes(), 0.0f } );
                if constexpr ( std::remove_reference_t<decltype( lin )>::kIsQuantized )
                    items.push_back( { flat + "." + sname, "F32", shapeOf( *lin.getWeightScale() ), lin.getWeightScale()->rawData(), lin.getWeightScale()->sizeInBytes(), 0.0f } );
            };
            auto addNorm = [&]( RmsNormType& n ) { items.push_back( { flatName( n.getName() ) + ".weight", "BF16", shapeOf( *n.getWeight() ), n.getWeight()->rawData(), n.getWeight()->sizeInBytes(), 0.0f } ); };
            addLinear( *lm_head_, "temb", "wte", "wte_scale" );      // the tied table under the embedding's name; no lm_head.weight
            for ( size_t i = 0; i < layers_.size(); ++i )
            {
                auto& L = layers_[ i ];
                addNorm( *L.input_norm ); addNorm( *L.q_norm ); addNorm( *L.k_norm ); addNorm( *L.v_norm ); addNorm( *L.post_attn_norm ); addNorm( *L.pre_ffn_norm ); addNorm( *L.post_ffn_norm );
                addLinear( *L.qkv_proj, flatName( L.qkv_proj->getName() ), "weight", "weight_scale" ); addLinear( *L.o_proj, flatName( L.o_proj->getName() ), "weight", "weight_scale" );
                addLinear( *L.fc_gate_up, flatName( L.fc_gate_up->getName() ), "weight", "weight_scale" ); addLinear( *L.fc_down, flatName( L.fc_down->getName() ), "weight", "weight_scale" );
                items.push_back( { "tf_layer_" + std::to_string( i ) + ".layer_scalar", "F32", { 1 }, nullptr, 4, L.layer_scalar } );
            }
            addNorm( *final_norm_ );
            return items;
        }
        std::string flatName( const std::string& component_name ) const
        {
            return component_name.compare( 0, name_.size() + 1, name_ + "." ) == 0 ? component_name.substr( name_.size() + 1 ) : component_name;
        }
        template<typename Writer> void writeItems( Writer& w, std::vector<SaveItem>& items )
        {
            w.beginData();
            std::vector<unsigned char> host;
            ctx_->synchronize();
            for ( auto& it : items )
            {
                if ( !it.dev ) { w.writeTensorData( it.name, &it.host_scalar, 4 ); continue; }
                host.resize( it.bytes );
                Compute::rocmCheck( mila_cdna4_memcpy_d2h( host.data(), it.dev, it.bytes, ctx_->getStream() ) );
                ctx_->synchronize();
                w.writeTensorData( it.name, host.data(), it.bytes );
            }
            w.close();
        }

    public:
        /// LanguageModel::savePretrained (Core/LanguageModel.ixx:116-148): every parameter in its STORAGE form (bf16, or e4m3 / packed e2m1 +
        /// fp32 scales) -- a quantized model writes a pre-quantized artifact that reloads without re-quantizing -- with the model description
        /// under __metadata__["mila_config"] and the policy under ["mila_quantization"]
        void saveSafeTensors( const std::string& path )
        {
            auto items = saveItems();
            Serialization::SafeTensorsWriter w( path );
            for ( auto& it : items ) w.declareTensor( it.name, it.dtype, it.shape );
            w.setMetadata( "format", "pt" );
            w.setMetadata( Serialization::kMilaQuantizationMetadataKey, weightQuantizationName() );
            w.setMetadata( Serialization::kMilaConfigMetadataKey, Serialization::toMetadataJSON( pretrainedMetadata() ) );
            writeItems( w, items );
        }
        /// the same tensors in the MILA .bin container (what the reference's converters emit and fromPretrained streams)
        void saveMilaBin( const std::string& path )
        {
            auto items = saveItems();
            Serialization::MilaBinWriter w( path );
            for ( auto& it : items ) w.declareTensor( it.name, it.dtype, it.shape );
            w.setMetadataJSON( Serialization::toMetadataJSON( pretrainedMetadata() ) );
            writeItems( w, items );
        }

        /// GemmaTransformer::loadParameters (Gemma.ixx:502-557): stream every blob of a MILA .bin or SafeTensors artifact in ascending file
        /// offset order into the component its flat name resolves to.  A Linear's `.weight` may be bf16 [N, K] (stored as is, or quantized
        /// on load under a quantized policy: Linear.ixx:529-558) or already in the policy's storage form with its `.weight_scale` sibling
        /// (:559-574); likewise `temb.wte` / `temb.wte_scale`.  The head is tied: it adopts the table, and an artifact that carries its own
        /// `lm_head.weight` is refused.  Unknown names, missing parameters, a geometry or policy that does not match this model: errors.
        void loadPretrained( const std::string& path )
        {
            destroyGraph();   // layer scalars are baked into the captured launches
            Compute::TraceRange tr( "gemma.loadPretrained" );
            Serialization::PretrainedModelReader r( path );
            const auto& md = r.getPretrainedMetadata();
            if ( !r.metadataJSON().empty() )
            {
                auto mismatch = [&]( const char* what, uint64_t file, uint64_t mine ) { if ( file != 0 && file != mine ) throw std::invalid_argument( "GemmaTransformer::loadPretrained: '" + path + "' declares " + what + " = " + std::to_string( file ) + ", this model has " + std::to_string( mine ) ); };
                mismatch( "vocab_size", md.vocab_size, (uint64_t)cfg_.vocab_size ); mismatch( "embedding_dim", md.embedding_dim, (uint64_t)cfg_.embedding_dim );
                mismatch( "num_layers", md.num_layers, (uint64_t)cfg_.num_layers ); mismatch( "hidden_dim", md.hidden_dim, (uint64_t)cfg_.hidden_dim );
                mismatch( "num_heads", md.num_heads, (uint64_t)cfg_.num_heads ); mismatch( "head_dim", md.head_dim, (uint64_t)cfg_.head_dim );
            }
            // a pre-quantized artifact loads only under the policy it was written with (GemmaModel.ixx:617-632)
            if ( !r.getWeightQuantization().empty() && r.getWeightQuantization() != weightQuantizationName() )
                throw std::runtime_error( "GemmaTransformer::loadPretrained: artifact '" + path + "' is pre-quantized as '" + r.getWeightQuantization() + "' but this model's policy is '" + weightQuantizationName() + "'" );
            using Entry = Serialization::SafeTensorsEntry;
            std::map<std::string, std::function<void( const Entry& )>> sinks;
            std::map<std::string, bool> required;
            auto bindLinear = [&]( auto& lin, const std::string& flat, const std::string& wname, const std::string& sname )
            {
                auto* lp = &lin;
                constexpr bool q = std::remove_reference_t<decltype( lin )>::kIsQuantized;
                sinks[ flat + "." + wname ] = [ lp ]( const Entry& e )
                {
                    const size_t NK = (size_t)lp->getConfig().getOutputFeatures() * lp->getConfig().getInputFeatures();
                    if ( e.dtype == "BF16" ) { if ( (size_t)e.elements() != NK ) throw std::invalid_argument( e.name + ": expected " + std::to_string( NK ) + " bf16 elements" ); }
                    else if ( !q || e.nbytes() != lp->getWeight().sizeInBytes() || ( e.dtype != "F8_E4M3" && e.dtype != "U8" ) )
                        throw std::invalid_argument( e.name + ": dtype " + e.dtype + " / " + std::to_string( e.nbytes() ) + " bytes does not fit this Linear's weight policy" );
                    lp->loadParameter( "weight", e.data, e.nbytes() );
                };
                required[ flat + "." + wname ] = false;
                if constexpr ( q )
                    sinks[ flat + "." + sname ] = [ lp ]( const Entry& e )
                    {
                        if ( e.dtype != "F32" ) throw std::invalid_argument( e.name + ": weight scales must be F32" );
                        lp->loadParameter( "weight_scale", e.data, e.nbytes() );
                    };
            };
            auto bindNorm = [&]( RmsNormType& n )
            {
                auto* np = &n;
                sinks[ flatName( n.getName() ) + ".weight" ] = [ np ]( const Entry& e )
                {
                    if ( e.dtype != "BF16" ) throw std::invalid_argument( e.name + ": norm weights must be BF16" );
                    np->loadParameter( "weight", e.data, e.nbytes() );
                };
                required[ flatName( n.getName() ) + ".weight" ] = false;
            };
            bindLinear( *lm_head_, "temb", "wte", "wte_scale" );
            for ( size_t i = 0; i < layers_.size(); ++i )
            {
                auto& L = layers_[ i ];
                bindNorm( *L.input_norm ); bindNorm( *L.q_norm ); bindNorm( *L.k_norm ); bindNorm( *L.v_norm ); bindNorm( *L.post_attn_norm ); bindNorm( *L.pre_ffn_norm ); bindNorm( *L.post_ffn_norm );
                for ( auto* lin : { L.qkv_proj.get(), L.o_proj.get(), L.fc_gate_up.get(), L.fc_down.get() } ) bindLinear( *lin, flatName( lin->getName() ), "weight", "weight_scale" );
                Layer* lp = &L;
                const std::string sn = "tf_layer_" + std::to_string( i ) + ".layer_scalar";
                sinks[ sn ] = [ lp ]( const Entry& e )
                {
                    if ( e.dtype != "F32" || e.elements() != 1 ) throw std::invalid_argument( e.name + ": layer_scalar must be one F32" );
                    std::memcpy( &lp->layer_scalar, e.data, 4 );
                };
                required[ sn ] = false;
            }
            bindNorm( *final_norm_ );
            std::vector<std::pair<std::string, std::string>> packed;     // storage-form tensor -> the scale sibling it needs
            const std::string prefix = name_ + ".";
            r.streamTensorBlobs( [&]( const std::string& full, const Entry& e )
            {
                const std::string flat = full.compare( 0, prefix.size(), prefix ) == 0 ? full.substr( prefix.size() ) : full;
                if ( flat == "lm_head.weight" || flat == "lm_head.weight_scale" )
                    throw std::invalid_argument( "GemmaTransformer::loadPretrained: '" + path + "' carries an untied '" + flat + "'; Gemma-4 ties the head to temb.wte (Gemma.ixx:540-555)" );
                auto it = sinks.find( flat );
                if ( it == sinks.end() ) throw std::invalid_argument( "GemmaTransformer::loadPretrained: '" + path + "' holds an unknown tensor '" + full + "'" );
                it->second( e );
                if ( required.count( flat ) ) required[ flat ] = true;
                const bool is_w = flat.size() > 7 && flat.compare( flat.size() - 7, 7, ".weight" ) == 0, is_t = flat == "temb.wte";
                if ( ( is_w || is_t ) && e.dtype != "BF16" ) packed.emplace_back( full, full + "_scale" );
            } );
            for ( auto& [ n, seen ] : required ) if ( !seen ) throw std::invalid_argument( "GemmaTransformer::loadPretrained: '" + path + "' lacks '" + n + "'" );
            for ( auto& [ n, sc ] : packed ) if ( !r.hasTensor( sc ) ) throw std::invalid_argument( "GemmaTransformer::loadPretrained: '" + n + "' is in storage form but '" + sc + "' is missing" );
            // op-owned derived state (fp4 tensor scale, resident prefill weights) once every sibling is in place, whatever the file order
            if constexpr ( TWeightQuant::kIsQuantized )
                for ( auto& L : layers_ )
                    for ( auto* lin : { L.qkv_proj.get(), L.o_proj.get(), L.fc_gate_up.get(), L.fc_down.get() } ) lin->getOperation().onQuantizedWeightsLoaded();
            ctx_->synchronize();
        }
        void loadSafeTensors( const std::string& path ) { loadPretrained( path ); }

        /// quantized policies: keep the prefill staging (fp8 -> bf16, fp4 -> e4m3) of every layer Linear resident (default on: +2 / +1
        /// bytes per weight of the 288 GB) or re-stage into scratch on every forward as the reference does; same bits
        void setResidentPrefillWeights( bool on )
        {
            for ( auto& L : layers_ )
                for ( auto* lin : { L.qkv_proj.get(), L.o_proj.get(), L.fc_gate_up.get(), L.fc_down.get() } ) lin->getOperation().setResidentPrefillWeights( on );
            ctx_->synchronize();
        }
        // ------------------------------------------------------------------------------------
        // footprint (Gemma.ixx:340-470): getMemoryStats() = what the model holds, getRequiredMemory() = what a model of this configuration, sequence length and
        // prefill chunk would hold once built and loaded -- computed from the configuration alone.  Two corrections as in the reference: the tied head reports the
        // shared table, subtracted once; every block reports one owner's RoPE tables, of which one pair per distinct geometry exists.
        // ------------------------------------------------------------------------------------
        MemoryStats getMemoryStats() const
        {
            MemoryStats st;
            std::map<const void*, std::pair<size_t, size_t>> rope;      // table -> (blocks sharing it, bytes one owner reports)
            for ( auto& L : layers_ )
            {
                st += L.getMemoryStats();
                auto& e = rope[ L.rope->getOperation().tableKey() ];
                e.first += 1; e.second = L.rope->getOperation().stateBytes();
            }
            for ( auto& [ key, e ] : rope ) st.device_state_bytes -= ( e.first - 1 ) * e.second;
            st += temb_->getMemoryStats();
            st += final_norm_->getMemoryStats();
            const MemoryStats head = lm_head_->getMemoryStats();
            st += head;
            st.device_parameter_bytes -= head.device_parameter_bytes;      // tied: the table is temb's
            st.device_state_bytes += ownStateBytes();
            return st;
        }
        MemoryStats getRequiredMemory() const
        {
            const dim_t D = cfg_.embedding_dim, P = max_prefill_;
            MemoryStats st;
            const BuildContext block_ctx( shape_t{ 1, P, D }, RuntimeMode::Inference );
            std::map<std::tuple<dim_t, uint32_t, dim_t>, std::pair<size_t, size_t>> rope;
            for ( auto& L : layers_ )
            {
                st += L.getRequiredMemory( block_ctx );
                uint32_t base_bits;
                const float base = L.rope->getConfig().getBase();
                std::memcpy( &base_bits, &base, 4 );
                auto& e = rope[ { L.rope->getConfig().getHeadDim(), base_bits, L.rope->getConfig().getRotaryDim() } ];
                e.first += 1; e.second = L.rope->getRequiredMemory( block_ctx ).device_state_bytes;
            }
            for ( auto& [ key, e ] : rope ) st.device_state_bytes -= ( e.first - 1 ) * e.second;
            st += temb_->getRequiredMemory( BuildContext( shape_t{ 1, P }, RuntimeMode::Inference ) );
            st += final_norm_->getRequiredMemory( BuildContext( shape_t{ 1, 1, D }, RuntimeMode::Inference ) );
            const MemoryStats head = lm_head_->getRequiredMemory( BuildContext( shape_t{ 1, 1, D }, RuntimeMode::Inference ) );
            st += head;
            st.device_parameter_bytes -= head.device_parameter_bytes;
            st.device_state_bytes += requiredOwnStateBytes();
            return st;
        }
    private:
        /// the transformer's own device buffers: the pooled block workspace, the prefill / fused-step scratch, logits, sampler and position words
        size_t ownStateBytes() const
        {
            size_t b = 0;
            for ( const auto& t : { q_, k_, v_, attn_out_, res1_, res2_, geglu_, blk_out_[ 0 ], blk_out_[ 1 ], ws_normed_, ws_o_normed_, ws_ffn_in_, ws_ffn_normed_, ws_q_normed_,
                                    ws_k_normed_, ws_v_normed_, ws_qkv_, ws_o_, ws_gate_up_, ws_down_ } ) b += tensorBytes( t );
            for ( const auto* t : { hidden_[ 0 ].get(), hidden_[ 1 ].get(), hidden_[ 2 ].get(), pf_x_[ 0 ].get(), pf_x_[ 1 ].get(), pf_norm_.get(), pf_norm2_.get(), pf_q8_[ 0 ].get(),
                                    pf_q8_[ 1 ].get(), f_qkv_.get(), f_q_.get(), f_o_.get(), f_down_.get(), f_act_.get(), ov_qkv_.get(), ov_o_.get(), ov_gate_up_.get() } ) b += tensorBytes( t );
            for ( const auto* t : { logits_.get(), sample_scratch_.get(), attn_partials_.get(), radix_scratch_.get(), pf_ts_[ 0 ].get(), pf_ts_[ 1 ].get() } ) b += tensorBytes( t );
            b += tensorBytes( pos_dev_.get() );
            b += rowsStateBytes();
            if ( lp_op_ ) b += lp_op_->stateBytes();
            if ( score_op_ ) b += score_op_->stateBytes();
            if ( token_table_ ) b += token_table_->stateBytes();
            if ( token_bias_ ) b += token_bias_->stateBytes();
            if ( token_automaton_ ) b += token_automaton_->stateBytes();
            if ( row_bias_ ) b += row_bias_->stateBytes();
            if ( row_automata_ ) b += row_automata_->stateBytes();
            if ( row_params_ ) b += row_params_->sizeInBytes();
            if ( row_masks_ ) b += row_masks_->sizeInBytes();
            return b;
        }
        size_t requiredOwnStateBytes() const
        {
            const size_t D = static_cast<size_t>( cfg_.embedding_dim ), P = static_cast<size_t>( max_prefill_ ), F = static_cast<size_t>( cfg_.hidden_dim );
            const size_t maxq = static_cast<size_t>( std::max( cfg_.qWidth( false ), cfg_.qWidth( true ) ) ), maxkv = static_cast<size_t>( std::max( cfg_.kvWidth( false ), cfg_.kvWidth( true ) ) );
            const size_t maxpacked = static_cast<size_t>( std::max( cfg_.packedQkvWidth( false ), cfg_.packedQkvWidth( true ) ) );
            size_t e = 0;      // bf16 elements
            e += P * ( maxq + 2 * maxkv + maxq + D + D + F + 2 * D );                                       // q k v attn_out res1 res2 geglu blk_out x 2
            e += P * ( 4 * D + maxq + 2 * maxkv + maxpacked + D + 2 * F + D );                              // the pooled role outputs
            e += 3 * D + 2 * P * D + 2 * P * D;                                                              // hidden x 3, pf_x x 2, pf_norm, pf_norm2
            if ( kFmt != 0 ) e += 2 * P * ( ( D + 1 ) / 2 );                                                 // per-token e4m3 rows of the fp8 x fp8 prefill paths
            e += maxpacked + maxq + D + D + F;                                                               // f_qkv f_q f_o f_down f_act
            size_t b = e * 2;
            if ( ov_qkv_ ) b += P * ( maxpacked + D + 2 * F ) * 2;                                           // the two-stream prefill's buffers, once that path has run
            b += static_cast<size_t>( cfg_.vocab_size ) * 4 + ( ( mila_cdna4_sample_scratch_bytes() / 4 ) * 4 ) + ( ( attnScratchBytes() + 3 ) / 4 ) * 4;
            b += ( ( mila_cdna4_sample_radix_scratch_bytes( (int)cfg_.vocab_size ) + 3 ) / 4 ) * 4;      // the radix sampler's workspace
            if ( kFmt != 0 ) b += 2 * P * 4;
            b += 4;                                                                                          // the device position word
            b += requiredRowsStateBytes();
            if ( lp_op_ ) b += lp_op_->stateBytes();                                                         // token log-probabilities, once setStepLogprobs() turned them on
            if ( score_op_ ) b += score_op_->stateBytes();                                                   // prompt log-probabilities, once prefillScored() has run
            if ( token_table_ ) b += Compute::RocmTokenTable::requiredBytes( cfg_.vocab_size, token_table_->rows() );      // the token tables, once a penalty was set
            if ( token_bias_ ) b += Compute::RocmTokenBias::requiredBytes( cfg_.vocab_size );                              // the bias table and its staging, once a bias was set
            if ( token_automaton_ ) b += token_automaton_->requiredBytes();                                              // the automaton's image, words and effective table, once one was set
            if ( row_bias_ ) b += Compute::RocmTokenBiasRows::requiredBytes( cfg_.vocab_size, static_cast<int>( cfg_.max_batch ) );      // row requests: the rows' tables, once one was set
            if ( row_automata_ ) b += row_automata_->requiredBytes();                                                    // ... the rows' images, words and descriptors
            if ( row_params_ ) b += mila_cdna4_sample_row_params_bytes( static_cast<int>( cfg_.max_batch ) );            // ... the rows' sampler records
            if ( row_masks_ ) b += 2 * static_cast<size_t>( cfg_.max_batch ) * 4;                                        // ... and the two masks per row
            return b;
        }
    public:
        /// bytes of op-owned prefill staging the layer Linears hold right now (fp8 policy: bf16 copies, 0 while the W8A8 prefill is on; fp4 policy: e4m3 copies)
        double residentStagingBytes() const
        {
            double b = 0;
            for ( auto& L : layers_ )
                for ( auto* lin : { L.qkv_proj.get(), L.o_proj.get(), L.fc_gate_up.get(), L.fc_down.get() } ) b += static_cast<double>( lin->getOperation().residentBytes() );
            return b;
        }
    private:
        std::string name_{ "gemma" };      // the root's name (metadata.model_name in the reference); dropped from flat tensor names
        GemmaConfig cfg_;
        dim_t max_seq_, max_prefill_;
        std::unique_ptr<IExecutionContext> owned_ctx_;
        Compute::RocmExecutionContext* ctx_{ nullptr };
        LayerList layers_;
        std::vector<mila_kv_fork_layer> fork_layers_;
        std::vector<mila_kv_fork_layer_fp8> fork_layers_fp8_;
        std::vector<mila_kv_fork_layer_band> fork_layers_band_;      // bounded_local_kv_rows: every layer, the sliding-window ones with their window
        dim_t ring_capacity_{ 0 };                                    // ... the ring layers' capacity (0: no ring rows)
        std::vector<dim_t> row_high_, row_from_;                      // ... per row (ringRows())
        std::shared_ptr<RmsNormType> final_norm_;
        std::shared_ptr<LmHeadLinearType> lm_head_;
        std::unique_ptr<TensorType> hidden_[ 3 ], pf_x_[ 2 ], f_qkv_, f_q_, f_o_, f_down_, f_act_;
        std::shared_ptr<TensorType> q_, k_, v_, attn_out_, res1_, res2_, geglu_, blk_out_[ 2 ];   // the blocks' shared workspace
        std::shared_ptr<TensorType> ws_normed_, ws_o_normed_, ws_ffn_in_, ws_ffn_normed_, ws_q_normed_, ws_k_normed_, ws_v_normed_, ws_qkv_, ws_o_, ws_gate_up_, ws_down_;   // ... one output per component role
        std::shared_ptr<TokenEmbeddingType> temb_;
        std::unique_ptr<LogitsTensor> logits_;
        std::unique_ptr<TokenTensor> pos_dev_;
        std::unique_ptr<LogitsTensor> sample_scratch_;
        bool sample_in_graph_{ false };
        bool fused_prefill_{ true };
        dim_t kv_fill_{ 0 };      ///< positions the caches hold, as far as eager calls tell (see rewindKvCache)
        bool prefill_overlap_{ false };
        std::unique_ptr<TensorType> ov_qkv_, ov_o_, ov_gate_up_;
        hipStream_t ov_stream_{ nullptr };
        hipEvent_t ov_ev_[ 8 ]{};
        std::unique_ptr<LogitsTensor> attn_partials_, radix_scratch_;
        std::unique_ptr<TensorType> pf_norm_, pf_norm2_;
        // W4A8 policy: the sandwich tails also write their normalised rows as per-token e4m3 + scales for the Linear that follows ([0]: pre_ffn_norm -> fc_gate_up,
        // [1]: the next block's input_norm -> its qkv_proj); model-owned like every prefill workspace
        std::unique_ptr<TensorType> pf_q8_[ 2 ];          // [1, P, D / 2] bf16 elements = P * D bytes of e4m3
        std::unique_ptr<LogitsTensor> pf_ts_[ 2 ];        // [P] fp32 per-token scales
        const uint16_t* cur_hidden_{ nullptr };
        std::unique_ptr<RowsState> rows_;               // max_batch > 1 or draft_tokens > 0 only
        hipGraph_t chain_graph_{ nullptr };
        hipGraphExec_t chain_graph_exec_{ nullptr };
        int chain_captured_T_{ 0 };
        dim_t chain_captured_band_{ 0 };
        size_t chain_graph_captures_{ 0 };
        hipGraph_t rows_graph_{ nullptr };
        hipGraphExec_t rows_graph_exec_{ nullptr };
        int rows_captured_B_{ 0 };
        bool rows_captured_greedy_{ false };
        dim_t rows_captured_band_{ 0 };
        size_t rows_graph_captures_{ 0 };
        // the stochastic tails of the rows / chain step: parameters + the device address of one draw per row, asked for and captured (nullopt / nullptr: none)
        std::optional<SamplingParams> rows_sampling_, rows_captured_sampling_, chain_sampling_, chain_captured_sampling_;
        const float* rows_draws_{ nullptr };
        const float* rows_captured_draws_{ nullptr };
        const float* chain_draws_{ nullptr };
        const float* chain_captured_draws_{ nullptr };
        hipGraph_t graph_{ nullptr };
        hipGraphExec_t graph_exec_{ nullptr };
        const int32_t* captured_token_{ nullptr };      // what the captured graph was built for: ensureGraph() re-captures on a mismatch
        dim_t captured_band_end_{ 0 };                  // ... and the live-length bucket (exclusive end) its attention launches were shaped for
        bool captured_sample_in_graph_{ false };
        size_t graph_captures_{ 0 };
        unsigned long long* token_ring_{ nullptr };
        unsigned long long* token_seq_{ nullptr };
        const unsigned long long* captured_ring_{ nullptr };
        int token_ring_size_{ 0 };
        std::optional<SamplingParams> graph_sampling_, captured_sampling_;      // the stochastic tail asked for / captured (nullopt: none)
        const float* draw_ring_{ nullptr };
        const float* captured_draw_ring_{ nullptr };
        int draw_ring_size_{ 0 };
        // token log-probabilities in the step: the setting asked for and what each of the three graphs was captured with; the op exists from the first enable on
        struct StepLogprobs
        {
            int top_n; uint32_t* ring; int ring_size;
            bool operator==( const StepLogprobs& ) const = default;
        };
        std::optional<StepLogprobs> step_lp_, captured_lp_, rows_captured_lp_, chain_captured_lp_;
        std::unique_ptr<Compute::RocmTokenLogprobsOp> lp_op_;
        std::unique_ptr<Compute::RocmLmHeadScoreOp> score_op_;
        // sampling filters: the greedy samplers' setting, what the one-row and the rows graph were captured with, and the token tables (from the first penalty on)
        SamplingParams filters_{}, captured_filters_{}, rows_captured_filters_{};
        std::unique_ptr<Compute::RocmTokenTable> token_table_;
        // logit bias: the table (from the first setTokenBias() on), whether it is on, and what the one-row and the rows graph were captured with
        std::unique_ptr<Compute::RocmTokenBias> token_bias_;
        bool bias_on_ = false, captured_bias_ = false, rows_captured_bias_ = false, chain_captured_bias_ = false;
        const float* biasValues() noexcept { return bias_on_ ? token_bias_->data() : nullptr; }
        // token automaton: the device side (from the first setTokenAutomaton() on), whether it is on, and what the one-row graph's step node was captured with
        std::unique_ptr<Compute::RocmTokenAutomaton> token_automaton_;
        bool automaton_on_ = false;
        std::optional<Compute::RocmTokenAutomaton::Key> captured_automaton_{}, chain_captured_automaton_{};
        std::optional<Compute::RocmTokenAutomaton::Key> automatonKey() const { return automaton_on_ ? std::optional( token_automaton_->key() ) : std::nullopt; }
        // row requests (mila_cdna4.h: row requests): the rows' sampler records on the device and their host mirror, the rows forms of the bias table and the
        // automaton (each from its first use on), and the class facts a rows graph was captured with -- parameters WITHIN a class are device words, not graph nodes
        struct RowsRequestKey
        {
            bool on = false, greedy_plain = false, greedy_constrained = false, stochastic = false, constrained = false, automaton = false, table = false;
            bool operator==( const RowsRequestKey& ) const = default;
        };
        // Two masks per row on the device, derived from the active word and the row's class: [ b ] = active and constrained (a bias or an automaton), [ max_batch + b ]
        // = active and unconstrained.  The greedy pair runs once per mask that has greedy rows: the constrained rows read their table over the CAPPED logits, the
        // plain rows take the logits as they are, as each does alone (the cap is monotone but can merge neighbours into a tie).  Updated wherever the active word or
        // a row's constraints change; allocated by the first setRowsRequests().
        std::unique_ptr<TokenTensor> row_masks_;
        std::vector<char> row_active_host_;
        void refreshRowMasks( int b )
        {
            if ( !row_masks_ ) return;
            if ( row_active_host_.empty() ) row_active_host_.assign( static_cast<size_t>( cfg_.max_batch ), 0 );      // (no row was ever activated: buildRows() left them inactive)
            const bool on = row_active_host_[ static_cast<size_t>( b ) ] != 0, c = rowConstrained( b );
            const int32_t w[ 2 ] = { on && c ? 1 : 0, on && !c ? 1 : 0 };
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( row_masks_->data() + b, &w[ 0 ], 4, ctx_->getStream() ) );
            Compute::rocmCheck( mila_cdna4_memcpy_h2d( row_masks_->data() + cfg_.max_batch + b, &w[ 1 ], 4, ctx_->getStream() ) );
            ctx_->synchronize();
        }
        std::unique_ptr<TokenTensor> row_params_;
        std::vector<SamplingParams> row_requests_;      // empty: the rows step takes the shared parameters, as ever
        std::vector<char> row_request_vacant_;          // beside row_requests_: 1 = a row below a setRowRequest row that has no request yet
        const float* row_request_draws_{ nullptr };
        std::unique_ptr<Compute::RocmTokenBiasRows> row_bias_;
        std::unique_ptr<Compute::RocmTokenAutomatonRows> row_automata_;
        RowsRequestKey rows_captured_key_{};
        bool rowConstrained( int b ) const { return ( row_bias_ && row_bias_->on( b ) ) || ( row_automata_ && row_automata_->on( b ) ); }
        RowsRequestKey rowsRequestKey() const
        {
            RowsRequestKey k{};
            if ( row_requests_.empty() ) return k;
            k.on = true;
            for ( size_t b = 0; b < row_requests_.size(); ++b )
            {
                if ( row_request_vacant_[ b ] ) continue;      // (setRowRequest: a row that never had a request carries no class)
                const bool greedy = !( row_requests_[ b ].temperature > 0.0f ), c = rowConstrained( static_cast<int>( b ) );
                if ( !greedy ) k.stochastic = true;
                else ( c ? k.greedy_constrained : k.greedy_plain ) = true;
                k.constrained = k.constrained || c;
                k.automaton = k.automaton || ( row_automata_ && row_automata_->on( static_cast<int>( b ) ) );
                k.table = k.table || row_requests_[ b ].penalized();
            }
            return k;
        }
        void noteRowActive( int b, bool on )
        {
            if ( row_active_host_.empty() ) row_active_host_.assign( static_cast<size_t>( cfg_.max_batch ), 0 );
            row_active_host_[ static_cast<size_t>( b ) ] = on ? 1 : 0;
            refreshRowMasks( b );
        }
        void ensureRowBias()
        {
            requireRows( 0 );
            if ( !row_bias_ ) row_bias_ = std::make_unique<Compute::RocmTokenBiasRows>( ctx_, cfg_.vocab_size, static_cast<int>( cfg_.max_batch ) );
        }
        /// what the one-row samplers read as their bias table: the automaton's effective table (composed over the bias table) while one is on
        const float* samplerBias() noexcept { return automaton_on_ ? token_automaton_->eff() : biasValues(); }
        void checkBiasEntries( const int32_t* ids, const float* values, size_t n, const char* who ) const
        {
            if ( n && ( !ids || !values ) ) throw std::invalid_argument( std::string( who ) + ": null pointer" );
            for ( size_t i = 0; i < n; ++i )
            {
                if ( ids[ i ] < 0 || ids[ i ] >= cfg_.vocab_size ) throw std::invalid_argument( std::string( who ) + ": token id " + std::to_string( ids[ i ] ) + " outside the vocabulary" );
                if ( std::isnan( values[ i ] ) || ( std::isinf( values[ i ] ) && values[ i ] > 0.0f ) )
                    throw std::invalid_argument( std::string( who ) + ": the value of id " + std::to_string( ids[ i ] ) + " must be finite or -inf" );
            }
        }
        static SamplingParams onlyFilters( const SamplingParams& f ) noexcept
        {
            SamplingParams o{};
            o.min_p = f.min_p; o.repetition_penalty = f.repetition_penalty; o.presence_penalty = f.presence_penalty; o.frequency_penalty = f.frequency_penalty;
            return o;
        }
        void ensureTokenTable()
        {
            // one table per batch row; a draft-token model's rows are positions of ONE sequence and its chain step takes no table: row 0 alone
            if ( !token_table_ ) token_table_ = std::make_unique<Compute::RocmTokenTable>( ctx_, cfg_.vocab_size, static_cast<int>( cfg_.max_batch > 1 ? cfg_.max_batch : 1 ) );
        }
        /// row `row`'s table words for a sampler with the filters `f`: nullptr without a penalty (min_p needs no table).  A capture never allocates: the setters did.
        uint32_t* tableWords( const SamplingParams& f, int row, bool may_allocate )
        {
            if ( !f.penalized() ) return nullptr;
            if ( may_allocate ) ensureTokenTable();
            if ( !token_table_ ) throw std::logic_error( "GemmaTransformer: penalties without a token table (setSamplingFilters / setGraphSampling / setRowsSampling allocate it)" );
            return token_table_->row( row );
        }
        /// what a GREEDY graph was captured for: min_p does not enter a greedy step
        static bool samePenalties( const SamplingParams& a, const SamplingParams& b ) noexcept
        {
            return a.repetition_penalty == b.repetition_penalty && a.presence_penalty == b.presence_penalty && a.frequency_penalty == b.frequency_penalty;
        }
        static bool sameFilters( const SamplingParams& a, const SamplingParams& b ) noexcept
        {
            return a.min_p == b.min_p && a.repetition_penalty == b.repetition_penalty && a.presence_penalty == b.presence_penalty && a.frequency_penalty == b.frequency_penalty;
        }
        static bool sameSampling( const std::optional<SamplingParams>& a, const std::optional<SamplingParams>& b ) noexcept
        {
            if ( a.has_value() != b.has_value() ) return false;
            return !a || ( a->temperature == b->temperature && a->top_k == b->top_k && a->top_p == b->top_p && sameFilters( *a, *b ) );
        }
    };
}
