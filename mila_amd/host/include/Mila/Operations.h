// Operation layer: OperationType, the OperationTraits primary template, and the CDNA4 (Rocm) op
// classes it resolves to.  Mirrors /root/reference/Mila/Src/Dnn/Compute/Operations/
// OperationTraits.Template.ixx:59-60,78-79,95-147, OperationType.ixx:29-49, OperationBase.ixx:21-175
// and is the build's counterpart of Compute/Devices/Cuda/Operations/OperationTraits.Cuda.ixx.
//
// Contract kept from the reference: ops are constructed by the component as
// std::make_shared<OpType>(IExecutionContext*, const Config&); they cache RAW pointers handed over by
// setParameters()/setWeightScales() and never own parameters; build() validates shapes and throws;
// forward() only enqueues work on the context's stream; scratch is fetched from the context on every
// forward.  A forward() is the C-ABI calls (include/mila_cdna4.h) of ONE route through its op, chosen in one place per op -- for a Linear of more than
// one row RocmLinearOp::route() / gegluRoute() -- and fails where no kernel serves the call: usually a single call; two where the route feeds the fp8
// matrix cores from bf16 rows (the per-token quantization launch, then the GEMM) or is the unfused Linear + GeGLU pair.
#pragma once

#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "Core.h"
#include "Quantization.h"

namespace Mila::Dnn::Compute
{
    enum class OperationType
    {
        LinearOp, GroupedQueryAttentionOp, MultiHeadAttentionOp, RmsNormOp, LayerNormOp, SoftmaxOp, GeluOp,
        GegluOp, SwigluOp, RopeOp, LpeOp, TokenEmbeddingOp, ResidualOp, SamplingOp,
    };

    /// primary stays undefined: a missing (Op, Device, Precision, Policy) row is a compile error
    template<OperationType TOp, DeviceType TDeviceType, TensorDataType TPrecision, typename TPolicy = void>
    struct OperationTraits;

    template<OperationType TOp, DeviceType TDeviceType, TensorDataType TPrecision, typename TPolicy = void>
    concept OperationSupported = requires { sizeof( OperationTraits<TOp, TDeviceType, TPrecision, TPolicy> ); };

    template<typename TOp, typename TTensor>
    concept UnaryOpConcept = requires( const TOp& op, const TTensor& in, TTensor& out ) { op.forward( in, out ); };

    template<typename TOp, typename TTensor>
    concept LinearOpConcept = requires( const TOp& op, const TTensor& in, TTensor& out ) { op.forward( in, out ); };

    /// Operation<Dev,Prec> base (OperationBase.ixx:21-175): holds the typed context
    template<DeviceType TDeviceType, TensorDataType TPrecision>
    class Operation
    {
    public:
        explicit Operation( IExecutionContext* ctx ) : context_( cast_context<TDeviceType>( ctx ) ) {}
        virtual ~Operation() = default;
        ExecutionContext<TDeviceType>* getExecutionContext() const noexcept { return context_; }
    protected:
        ExecutionContext<TDeviceType>* context_;
    };

    using RocmBf16Tensor = Tensor<TensorDataType::BF16, RocmDeviceMemoryResource>;
    template<TensorDataType TPrecision> using RocmTensor = Tensor<TPrecision, RocmDeviceMemoryResource>;
    /// the precisions the CDNA4 op rows exist for: BF16 (the product path) and FP32 (the reference's "validation and reference" rows, OperationTraits.Cuda.ixx:50-54,
    /// :108-126, :274-282 -- Linear, LayerNorm, Softmax, GELU, Residual, MHA, LPE, RoPE, RMSNorm; csrc/fp32_rows.hip)
    template<TensorDataType TPrecision> concept RocmPrecision = TPrecision == TensorDataType::BF16 || TPrecision == TensorDataType::FP32;

    // ---------------------------------------------------------------------------------------
    // Linear
    // ---------------------------------------------------------------------------------------
    struct LinearOpConfig
    {
        dim_t in_features{ 0 }, out_features{ 0 };
        bool has_bias{ false };
    };

    /// Test instrument (off unless a test installs one): records the per-token e4m3 activations a Linear on an fp8 x fp8 prefill path (W4A8, W8A8) consumed -- the bytes
    /// and the scales, copied to the host behind a stream synchronize.  A teacher-forced oracle then multiplies THOSE bytes layer by layer, so that a whole-model logit
    /// comparison is not at the mercy of e4m3 code flips upstream (tests/test_gemma_conditioned_gpu.py).  One pointer test per forward when off.
    struct ActivationTap
    {
        struct Record { int M, K, N; std::vector<uint8_t> x8; std::vector<float> ts; };
        std::vector<Record> records;
    };
    inline ActivationTap*& activationTap() { static ActivationTap* tap = nullptr; return tap; }

    /// What serves a Linear call of more than one row.  RocmLinearOp::route() is the only place that decides it: forward(), acceptsFp8Activations(),
    /// forwardFp8Activations() and usesContextScratch() read the answer.
    enum class PrefillRoute
    {
        Bf16,            ///< the bf16 GEMM on the op's own weights, the context scratch as its split-K workspace (unquantized weights)
        ResidentBf16,    ///< the same GEMM on the bf16 copy staged at load (fp8 policy)
        Staged,          ///< the _staged entry: dequantize into scratch, then the bf16 GEMM; a scratch need of 0 is the in-register dequantizing kernel
        Fp8Rows,         ///< fp8 x fp8 on per-token e4m3 rows: W8A8 on the policy's own weights (fp8 policy), W4A8 on the resident e4m3 copy (fp4 policy)
        W4a8OneCall,     ///< gemm_bf16_w4a8: the weights and the rows staged into scratch inside the one call (fp4 policy without the resident copy)
    };
    /// ... and what serves Linear + GeGLU (RocmLinearOp::gegluRoute(), read by forwardGeglu(), gegluWantsFp8Rows() and gegluUsesContextScratch()): one fused kernel
    /// on the weights the matching PrefillRoute reads, or the pair forward() + geglu_bf16
    enum class GegluRoute { FusedBf16, FusedResidentBf16, FusedStaged, FusedFp8Rows, FusedW4a8OneCall, Pair };

    /// counterpart of CudaLinearOp<Prec, TWeightQuant> (OPS/Linear/CudaLinearOp.ixx:107-1287)
    template<TensorDataType TPrecision, Quant::Weight::WeightQuantPolicy TWeightQuant>
    class RocmLinearOp : public Operation<DeviceType::Rocm, TPrecision>
    {
        static_assert( TPrecision == TensorDataType::BF16 || ( TPrecision == TensorDataType::FP32 && !TWeightQuant::kIsQuantized ),
                       "the CDNA4 Linear rows: BF16 activations under every weight policy, FP32 with unquantized weights (the validation row)" );
    public:
        using TensorType = RocmTensor<TPrecision>;
        static constexpr bool kFp32 = TPrecision == TensorDataType::FP32;
        static constexpr int kFmt = Quant::Weight::abiWeightFormat<TWeightQuant>();
        static constexpr int kGroup = Quant::Weight::groupSizeOf<TWeightQuant>();

        RocmLinearOp( IExecutionContext* ctx, const LinearOpConfig& cfg ) : Operation<DeviceType::Rocm, TPrecision>( ctx ), cfg_( cfg )
        {
            if ( cfg.in_features <= 0 || cfg.out_features <= 0 ) throw std::invalid_argument( "RocmLinearOp: feature counts must be positive" );
            if constexpr ( kFmt == 2 )
                if ( cfg.in_features % kGroup != 0 ) throw std::invalid_argument( "RocmLinearOp: in_features must be a multiple of the FP4 group size" );
        }

        /// caches raw pointers; never owns (OperationBase.ixx:52-64, CudaLinearOp.ixx:192-241)
        void setParameters( ITensor* weight, ITensor* bias )
        {
            if ( !weight ) throw std::invalid_argument( "RocmLinearOp::setParameters: weight is required" );
            if ( cfg_.has_bias && !bias ) throw std::invalid_argument( "RocmLinearOp::setParameters: bias is required by the config" );
            weight_ = weight->rawData();
            bias_ = bias ? static_cast<const uint16_t*>( bias->rawData() ) : nullptr;      // (FP32 row: float elements behind the same pointer)
        }

        void setWeightScales( ITensor* scales )
        {
            if constexpr ( !TWeightQuant::kIsQuantized ) throw std::logic_error( "RocmLinearOp::setWeightScales: policy is not quantized" );
            if ( !scales ) throw std::invalid_argument( "RocmLinearOp::setWeightScales: null scales" );
            scales_ = static_cast<const float*>( scales->rawData() );
        }

        void build( const BuildContext& ctx )
        {
            const auto& s = ctx.inputShape();
            if ( s.back() != cfg_.in_features )
                throw std::invalid_argument( "RocmLinearOp::build: input feature dimension " + std::to_string( s.back() ) +
                                             " does not match in_features " + std::to_string( cfg_.in_features ) );
            if ( !weight_ ) throw std::runtime_error( "RocmLinearOp::build: setParameters() must be called first" );
            if ( TWeightQuant::kIsQuantized && !scales_ ) throw std::runtime_error( "RocmLinearOp::build: setWeightScales() must be called first" );
            built_ = true;
        }

        /// The one decision of a call of M > 1 rows.
        /// fp8 policy: W8A8 when opted in (setFp8ActivationPrefill) -- "FP8 matmul consumes weights and scales natively" (Quantization/Weight/Policies.ixx:39-40) --, else
        /// the resident bf16 copy where the staged call would dequantize (the LDS-DMA GEMM applies), else the staged entry.
        /// fp4 policy: W4A8, the reference's default prefill for it (kUseFp8ActivationPrefillPath, CudaLinearOp.ixx:646-715), on the resident e4m3 copy or staged inside
        /// the one call; it needs the per-tensor weight scale, else the staged W4A16 entry.
        PrefillRoute route( int M ) const
        {
            if constexpr ( kFmt == 0 ) return PrefillRoute::Bf16;
            if ( fp8Serves( M ) && ( kFmt == 1 || weight_fp8_scale_ ) ) return ( kFmt == 1 || resident_e4m3_ ) ? PrefillRoute::Fp8Rows : PrefillRoute::W4a8OneCall;
            if ( resident_bf16_ && mila_cdna4_gemm_staging_bytes( M, (int)cfg_.in_features, (int)cfg_.out_features ) != 0 ) return PrefillRoute::ResidentBf16;
            return PrefillRoute::Staged;
        }
        /// bytes of context scratch forward() of M > 1 rows takes on route r: staging, per-token activation rows, a split-K workspace
        size_t scratchBytes( PrefillRoute r, int M ) const
        {
            const int K = (int)cfg_.in_features, N = (int)cfg_.out_features;
            switch ( r )
            {
            case PrefillRoute::Staged: return mila_cdna4_gemm_staging_bytes( M, K, N );
            case PrefillRoute::Fp8Rows: return activationBytes( M, K ) + mila_cdna4_gemm_fp8_workspace_bytes( M, K, N );
            case PrefillRoute::W4a8OneCall: return mila_cdna4_gemm_w4a8_scratch_bytes( M, K, N );
            default: return mila_cdna4_gemm_workspace_bytes( M, K, N );
            }
        }
        /// true when forward() of M rows takes anything from the context scratch (one call at a time may: two calls on two streams would share it).  The staged entry
        /// of an op without a resident copy counts whatever the shape: it dequantizes into scratch wherever the plan streams bf16 weights, and only a plan of 128-tile
        /// kernels alone needs no bytes -- a caller that asks for some row counts must not conclude from those that the op never stages.  (With the resident copy the
        /// route is Staged only where that need is 0.)
        bool usesContextScratch( int M ) const
        {
            if ( M <= 1 ) return false;
            const PrefillRoute r = route( M );
            return ( r == PrefillRoute::Staged && !resident_bf16_ ) || scratchBytes( r, M ) != 0;
        }

        /// M == 1 -> decode matvec; M > 1 -> the GEMM of route( M ) (CudaLinearOp.ixx:535-827)
        void forward( const TensorType& in, TensorType& out ) const
        {
            if ( !built_ ) throw std::runtime_error( "RocmLinearOp::forward: not built" );
            const int K = narrowToKernelIndex( cfg_.in_features, "in_features" );
            const int N = narrowToKernelIndex( cfg_.out_features, "out_features" );
            const int M = narrowToKernelIndex( static_cast<dim_t>( in.size() ) / cfg_.in_features, "outer size" );
            mila_stream_t st = this->context_->getStream();
            if constexpr ( kFp32 )
            {
                // the FP32 row (CudaMatVecBias.Fp32.cu:40, CudaMatMulFp32.cu:31-183): fp32 in / accumulate / out
                auto* yf = static_cast<float*>( out.rawData() );
                auto* xf = static_cast<const float*>( in.rawData() );
                const auto* wf = static_cast<const float*>( weight_ );
                const auto* bf = reinterpret_cast<const float*>( bias_ );
                if ( M == 1 ) rocmCheck( mila_cdna4_matvec_fp32( yf, xf, wf, bf, K, N, st ) );
                else rocmCheck( mila_cdna4_gemm_fp32( yf, xf, wf, bf, M, K, N, 0, st ) );
                return;
            }
            auto* y = static_cast<uint16_t*>( out.rawData() );
            auto* x = static_cast<const uint16_t*>( in.rawData() );
            if ( M == 1 ) { matvec( y, x ); return; }
            const auto* w8 = static_cast<const uint8_t*>( weight_ );
            const PrefillRoute r = route( M );
            switch ( r )
            {
            case PrefillRoute::Bf16: gemmWithWorkspace( y, x, static_cast<const uint16_t*>( weight_ ), M, K, N, 0, st ); break;
            // resident prefill weights: the staging pass was run once, at load (same values => same bits as the staged call)
            case PrefillRoute::ResidentBf16: gemmWithWorkspace( y, x, resident_bf16_->data(), M, K, N, 0, st ); break;
            case PrefillRoute::Staged:
            {
                // 2-phase staging through context scratch when the LDS-DMA GEMM applies; scratch is fetched per forward and never cached (reference rule,
                // CudaLinearOp.ixx:603-614)
                const size_t need = scratchBytes( r, M );
                void* scratch = need ? this->context_->getScratch( need ) : nullptr;
                if constexpr ( kFmt == 1 ) rocmCheck( mila_cdna4_gemm_bf16_w8a16_staged( y, x, w8, scales_, bias_, M, K, N, scratch, need, st ) );
                else rocmCheck( mila_cdna4_gemm_bf16_w4a16_staged( y, x, w8, scales_, bias_, M, K, N, kGroup, scratch, need, st ) );
                break;
            }
            case PrefillRoute::Fp8Rows:
            {
                // per-token e4m3 activations + the fp8 x fp8 MFMA GEMM: no staging pass, no bf16 copy of the weights
                uint8_t* x8; float* ts; void* ws;
                const size_t ws_bytes = mila_cdna4_gemm_fp8_workspace_bytes( M, K, N );
                activationScratch( M, K, x8, ts, ws_bytes, &ws );
                rocmCheck( mila_cdna4_quantize_fp8_per_token( x8, ts, x, M, K, st ) );
                recordTap( x8, ts, M, K, N );
                gemmFp8Rows( y, x8, ts, M, K, N, ws, ws_bytes, st );
                break;
            }
            case PrefillRoute::W4a8OneCall:
            {
                const size_t need = scratchBytes( r, M );
                rocmCheck( mila_cdna4_gemm_bf16_w4a8( y, x, w8, scales_, weight_fp8_scale_->data(), bias_, M, K, N, kGroup, this->context_->getScratch( need ), need, st ) );
                break;
            }
            }
        }
        /// the decode matvec of this op's weights: y[N] = W x[K] (+ bias); forward()'s M == 1 branch, and the o_proj / fc_down launches of the fused decode step
        void matvec( uint16_t* y, const uint16_t* x ) const
        {
            const int K = (int)cfg_.in_features, N = (int)cfg_.out_features;
            mila_stream_t st = this->context_->getStream();
            if constexpr ( kFmt == 0 ) rocmCheck( mila_cdna4_matvec_bf16( y, x, static_cast<const uint16_t*>( weight_ ), bias_, K, N, st ) );
            else if constexpr ( kFmt == 1 ) rocmCheck( mila_cdna4_matvec_bf16_qfp8( y, x, static_cast<const uint8_t*>( weight_ ), scales_, bias_, K, N, st ) );
            else rocmCheck( mila_cdna4_matvec_bf16_qfp4( y, x, static_cast<const uint8_t*>( weight_ ), scales_, bias_, K, N, kGroup, st ) );
        }

        /// matvec() for `rows` (2 .. 4) independent input vectors from ONE pass over the weights (mila_cdna4_matvec_rows): row b reads x + b * x_stride and writes
        /// y + b * y_stride (elements); row b has the bits matvec() gives on that row alone.  The o_proj / fc_down launches of the rows decode step
        void matvecRows( uint16_t* y, const uint16_t* x, int rows, int64_t x_stride, int64_t y_stride ) const
        {
            mila_matvec_rows_args r{};
            r.a.y = y; r.a.x = x; r.a.W = weight_; r.a.scales = scales_; r.a.post_scale = 1.0f; r.a.fmt = kFmt;
            r.a.K = (int)cfg_.in_features; r.a.N = (int)cfg_.out_features; r.a.group = kFmt == 2 ? kGroup : 0;
            r.bias = bias_; r.rows = rows; r.x_stride = x_stride; r.y_stride = y_stride;
            rocmCheck( mila_cdna4_matvec_rows( &r, this->context_->getStream() ) );
        }

        /// true when forwardGelu() serves this op and row count: unquantized weights on the GEMM branch
        bool fusesGelu( dim_t rows ) const noexcept { return kFmt == 0 && rows > 1; }

        /// Linear -> tanh-GELU in one kernel (the MLP's fc_1 -> gelu, MLP.ixx:148-161): the bits of forward() followed by RocmGeluOp::forward()
        void forwardGelu( const TensorType& in, TensorType& out ) const
        {
            if ( !built_ ) throw std::runtime_error( "RocmLinearOp::forwardGelu: not built" );
            const int K = narrowToKernelIndex( cfg_.in_features, "in_features" );
            const int N = narrowToKernelIndex( cfg_.out_features, "out_features" );
            const int M = narrowToKernelIndex( static_cast<dim_t>( in.size() ) / cfg_.in_features, "outer size" );
            if ( !fusesGelu( M ) ) throw std::logic_error( "RocmLinearOp::forwardGelu: only unquantized weights at more than one row" );
            if constexpr ( kFp32 )
                rocmCheck( mila_cdna4_gemm_fp32( static_cast<float*>( out.rawData() ), static_cast<const float*>( in.rawData() ), static_cast<const float*>( weight_ ),
                                                 reinterpret_cast<const float*>( bias_ ), M, K, N, 1, this->context_->getStream() ) );
            else if constexpr ( kFmt == 0 )
                gemmWithWorkspace( static_cast<uint16_t*>( out.rawData() ), static_cast<const uint16_t*>( in.rawData() ), static_cast<const uint16_t*>( weight_ ), M, K, N, 1,
                                   this->context_->getStream() );
        }

        /// The one decision of Linear + GeGLU over M > 1 rows of a [2F, K] = [gate | up] weight.  Two things are not what the Linear's own route would suggest:
        /// once the fp8 x fp8 path serves the shape no bf16 fused form is taken, even where the fp8 GeGLU kernel does not apply (the plain fp8 GEMM would split K) --
        /// the pair runs, and forward() takes the fp8 path; and under the fp4 policy that holds without the per-tensor weight scale too, where forward() then stages W4A16.
        GegluRoute gegluRoute( int M ) const
        {
            const int K = (int)cfg_.in_features, F = (int)cfg_.out_features / 2;
            if ( kFmt != 0 && fp8Serves( M ) )
            {
                if ( !mila_cdna4_gemm_geglu_w4a8_applicable( M, K, F ) || !( kFmt == 1 || weight_fp8_scale_ ) ) return GegluRoute::Pair;
                return ( kFmt == 1 || resident_e4m3_ ) ? GegluRoute::FusedFp8Rows : GegluRoute::FusedW4a8OneCall;
            }
            // the fused bf16 forms where they are also the faster choice for a caller that holds the split-K workspace, as forward() does
            if ( !mila_cdna4_gemm_geglu_preferred( M, K, F ) ) return GegluRoute::Pair;
            if constexpr ( kFmt == 0 ) return GegluRoute::FusedBf16;
            return resident_bf16_ ? GegluRoute::FusedResidentBf16 : GegluRoute::FusedStaged;
        }
        /// true when forwardGeglu() of M rows wants them quantized per token by their producer (x8 / ts): the quantization launch is then skipped, same bits
        bool gegluWantsFp8Rows( int M ) const { return gegluRoute( M ) == GegluRoute::FusedFp8Rows; }
        /// usesContextScratch() for forwardGeglu() (the fp8 x fp8 form counted as quantizing its rows itself)
        bool gegluUsesContextScratch( int M ) const
        {
            const GegluRoute r = gegluRoute( M );
            return r == GegluRoute::Pair ? usesContextScratch( M ) : r != GegluRoute::FusedBf16 && r != GegluRoute::FusedResidentBf16;
        }

        /// act[M, F] = GeGLU( forward( in ) ) (the FFN's fc_gate_up -> geglu): one kernel where gegluRoute() names a fused form -- the [M, 2F] gate | up rows then never
        /// reach memory --, else forward() into `gate_up` + geglu_bf16.  The bits of the pair either way.  x8 / ts: `in`'s rows as the producing kernel quantized them
        /// (caller-owned, only where gegluWantsFp8Rows()).
        void forwardGeglu( const TensorType& in, TensorType& act, TensorType& gate_up, const uint8_t* x8 = nullptr, const float* ts = nullptr ) const requires ( !kFp32 )
        {
            if ( !built_ ) throw std::runtime_error( "RocmLinearOp::forwardGeglu: not built" );
            const int K = narrowToKernelIndex( cfg_.in_features, "in_features" ), F = narrowToKernelIndex( cfg_.out_features / 2, "half of out_features" );
            const int M = narrowToKernelIndex( static_cast<dim_t>( in.size() ) / cfg_.in_features, "outer size" );
            mila_stream_t st = this->context_->getStream();
            auto* y = act.data();
            const auto* x = in.data();
            const auto* w8 = static_cast<const uint8_t*>( weight_ );
            const GegluRoute r = gegluRoute( M );
            if ( ( x8 || ts ) && ( r != GegluRoute::FusedFp8Rows || !x8 || !ts ) ) throw std::logic_error( "RocmLinearOp::forwardGeglu: quantized rows handed to a call that does not consume them" );
            if ( bias_ && r != GegluRoute::Pair ) throw std::logic_error( "RocmLinearOp::forwardGeglu: the fused Linear + GeGLU kernels take no bias" );
            if ( cfg_.out_features % 2 != 0 || act.size() < static_cast<size_t>( M ) * F || ( r == GegluRoute::Pair && gate_up.size() < static_cast<size_t>( M ) * 2 * F ) )
                throw std::invalid_argument( "RocmLinearOp::forwardGeglu: act must hold [M, F] and gate_up [M, 2F] elements of an even out_features" );
            switch ( r )
            {
            case GegluRoute::FusedBf16: rocmCheck( mila_cdna4_gemm_geglu_bf16( y, x, static_cast<const uint16_t*>( weight_ ), M, K, F, st ) ); break;
            case GegluRoute::FusedResidentBf16: rocmCheck( mila_cdna4_gemm_geglu_bf16( y, x, resident_bf16_->data(), M, K, F, st ) ); break;
            case GegluRoute::FusedStaged:
            {
                const size_t need = (size_t)2 * F * K * 2;
                void* scratch = this->context_->getScratch( need );
                if constexpr ( kFmt == 1 ) rocmCheck( mila_cdna4_gemm_geglu_bf16_w8a16_staged( y, x, w8, scales_, M, K, F, scratch, need, st ) );
                else rocmCheck( mila_cdna4_gemm_geglu_bf16_w4a16_staged( y, x, w8, scales_, M, K, F, kGroup, scratch, need, st ) );
                break;
            }
            case GegluRoute::FusedFp8Rows:
                if ( !x8 )
                {
                    uint8_t* q; float* s;
                    activationScratch( M, K, q, s );
                    rocmCheck( mila_cdna4_quantize_fp8_per_token( q, s, x, M, K, st ) );
                    x8 = q; ts = s;
                }
                // W8A8: the policy's e4m3 [2F, K] weights and per-channel scales; W4A8: the resident e4m3 copy and the per-tensor scale
                if constexpr ( kFmt == 1 ) rocmCheck( mila_cdna4_gemm_geglu_fp8_w8a8( y, x8, w8, ts, scales_, M, K, F, st ) );
                else rocmCheck( mila_cdna4_gemm_geglu_fp8_scaled( y, x8, resident_e4m3_->data(), ts, weight_fp8_scale_->data(), M, K, F, st ) );
                break;
            case GegluRoute::FusedW4a8OneCall:
            {
                const size_t need = mila_cdna4_gemm_w4a8_scratch_bytes( M, K, 2 * F );
                rocmCheck( mila_cdna4_gemm_geglu_bf16_w4a8( y, x, w8, scales_, weight_fp8_scale_->data(), M, K, F, kGroup, this->context_->getScratch( need ), need, st ) );
                break;
            }
            case GegluRoute::Pair:
                forward( in, gate_up );
                rocmCheck( mila_cdna4_geglu_bf16( y, gate_up.data(), M, F, st ) );
                break;
            }
        }

        /// the bf16 GEMM with the context's scratch as its workspace, as CudaLinearOp hands context_->getCublasLtWorkspace() to every plan (CudaLinearOp.ixx:637-638,
        /// :817-818): short prompts and remainders split K through it.  Fetched per forward, never cached.
        void gemmWithWorkspace( uint16_t* y, const uint16_t* x, const uint16_t* w, int M, int K, int N, int act, mila_stream_t st ) const
        {
            const size_t need = mila_cdna4_gemm_workspace_bytes( M, K, N );
            void* ws = need ? this->context_->getScratch( need ) : nullptr;
            rocmCheck( mila_cdna4_gemm_bf16_ws( y, x, w, bias_, M, K, N, act, ws, need, st ) );
        }

        void backward( const TensorType&, const TensorType&, TensorType& ) const
        {
            throw std::logic_error( "RocmLinearOp::backward: the CDNA4 backend is inference-only (and the reference forbids backward on quantized weights)" );
        }

        /// quantize-on-load: bf16 source already on the device (CudaLinearOp.ixx:332-392)
        void quantize( const uint16_t* src_bf16_device, ITensor& weight_out, ITensor& scales_out ) const
        {
            const int K = narrowToKernelIndex( cfg_.in_features, "in_features" );
            const int N = narrowToKernelIndex( cfg_.out_features, "out_features" );
            mila_stream_t st = this->context_->getStream();
            if constexpr ( kFmt == 1 )
                rocmCheck( mila_cdna4_quantize_fp8_per_channel( static_cast<uint8_t*>( weight_out.rawData() ), static_cast<float*>( scales_out.rawData() ), src_bf16_device, N, K, st ) );
            else if constexpr ( kFmt == 2 )
                rocmCheck( mila_cdna4_quantize_fp4_per_group( static_cast<uint8_t*>( weight_out.rawData() ), static_cast<float*>( scales_out.rawData() ), src_bf16_device, N, K, kGroup, st ) );
            else
                throw std::logic_error( "RocmLinearOp::quantize: NoWeightQuant has no quantize path" );
        }

        /// fp4 policy: (re)compute the per-tensor e4m3 weight scale the W4A8 prefill needs (an op-owned device scalar, like
        /// CudaLinearOp's weight_fp8_scale_, CudaLinearOp.ixx:311-330, :1118-1129)
        void onQuantizedWeightsLoaded()
        {
            if constexpr ( kFmt == 2 )
            {
                if ( !scales_ ) return;
                if ( !weight_fp8_scale_ ) weight_fp8_scale_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( this->context_->getDeviceId(), shape_t{ 1 } );
                rocmCheck( mila_cdna4_fp4_weight_fp8_scale( weight_fp8_scale_->data(), scales_, (int64_t)cfg_.out_features * ( cfg_.in_features / kGroup ), this->context_->getStream() ) );
            }
            refreshResident();
        }
        /// Resident prefill weights (default on): the staging pass of the quantized prefill -- fp8 -> bf16 (W8A16), fp4 -> e4m3 (W4A8) --
        /// is run ONCE when the weights are loaded and kept in an op-owned tensor (+2 / +1 bytes per weight), instead of into context
        /// scratch on every forward as the reference must on a 12 GB card (CudaLinearOp.ixx:597-644, :646-715).  Decode still streams the
        /// quantized weights; prefill results are bit-identical either way.
        void setResidentPrefillWeights( bool on )
        {
            resident_ = on;
            if ( !on ) { resident_bf16_.reset(); resident_e4m3_.reset(); }
            else refreshResident();
        }
        bool residentPrefillWeights() const noexcept { return resident_; }
        /// true when forward() of M rows runs fp8 x fp8 on per-token e4m3 rows: a producer may then hand over its output already quantized per token
        /// (forwardFp8Activations) instead of as bf16
        bool acceptsFp8Activations( int M ) const { return route( M ) == PrefillRoute::Fp8Rows; }
        /// forward() on activations the caller quantized (x8 [M, K] e4m3, ts [M] per-token scales -- exactly what quantize_fp8_per_token gives): the same GEMM call
        /// forward() makes, so the output carries the same bits
        /// (x8 / ts are the caller's own buffers, NOT context scratch: the GEMM's split-K workspace is taken from there)
        void forwardFp8Activations( const uint8_t* x8, const float* ts, uint16_t* y, int M ) const
        {
            if ( !acceptsFp8Activations( M ) ) throw std::logic_error( "RocmLinearOp::forwardFp8Activations: the fp8 x fp8 path does not serve this call" );
            const int K = (int)cfg_.in_features, N = (int)cfg_.out_features;
            const size_t ws_bytes = mila_cdna4_gemm_fp8_workspace_bytes( M, K, N );
            gemmFp8Rows( y, x8, ts, M, K, N, ws_bytes ? this->context_->getScratch( ws_bytes ) : nullptr, ws_bytes, this->context_->getStream() );
        }
        /// fp4 policy: W4A8 prefill (default on, as in the reference) or the dequantize -> bf16 GEMM fallback.
        /// fp8 policy: W8A8 prefill (default OFF: the reference's arithmetic for PerChannelFp8<> is W8A16, CudaLinearOp.ixx:597-644) -- the policy's e4m3 weights and
        /// per-channel scales consumed by the fp8 matrix cores where they lie (Policies.ixx:39-40); while it is on the op holds no bf16 copy of its weights
        void setFp8ActivationPrefill( bool on )
        {
            use_fp8_activation_prefill_ = on;
            if constexpr ( kFmt == 1 )
            {
                if ( on ) resident_bf16_.reset();
                else refreshResident();
            }
        }
        bool fp8ActivationPrefill() const noexcept { return use_fp8_activation_prefill_; }

        /// bytes of the op-owned resident staging (0 when off, when W8A8 is on, or for unquantized weights)
        size_t residentBytes() const noexcept { return ( resident_bf16_ ? resident_bf16_->size() * 2 : 0 ) + ( resident_e4m3_ ? resident_e4m3_->size() : 0 ); }
        /// op-owned device state right now: the resident staging + the fp4 policy's per-tensor e4m3 scale (CudaLinearOp.ixx:1118-1129 owns the same scalar)
        size_t stateBytes() const noexcept { return residentBytes() + ( weight_fp8_scale_ ? sizeof( float ) : 0 ); }
        /// ... and once quantized weights are in place, under the current switches (getRequiredStateMemorySize of the reference's ops)
        size_t requiredStateBytes() const noexcept
        {
            const size_t N = static_cast<size_t>( cfg_.out_features ), K = static_cast<size_t>( cfg_.in_features );
            if constexpr ( kFmt == 1 ) return ( resident_ && !use_fp8_activation_prefill_ ) ? N * K * 2 : 0;
            else if constexpr ( kFmt == 2 ) return sizeof( float ) + ( ( resident_ && K % 32 == 0 ) ? N * K : 0 );
            else return 0;
        }
        const void* weightPtr() const noexcept { return weight_; }
        const float* scalesPtr() const noexcept { return scales_; }
        const LinearOpConfig& config() const noexcept { return cfg_; }

    private:
        LinearOpConfig cfg_;
        const void* weight_{ nullptr };
        const uint16_t* bias_{ nullptr };
        const float* scales_{ nullptr };
        bool built_{ false };
        bool use_fp8_activation_prefill_{ kFmt == 2 };
        bool resident_{ true };
        std::unique_ptr<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>> weight_fp8_scale_;
        std::unique_ptr<RocmBf16Tensor> resident_bf16_;      // (quantized policies exist for BF16 activations only)
        std::unique_ptr<Tensor<TensorDataType::FP8_E4M3, RocmDeviceMemoryResource>> resident_e4m3_;

        /// the fp8 x fp8 prefill is switched on and an fp8 MFMA kernel serves M rows of this [N, K] weight
        bool fp8Serves( int M ) const { return use_fp8_activation_prefill_ && mila_cdna4_gemm_fp8_applicable( M, (int)cfg_.in_features, (int)cfg_.out_features ) != 0; }
        /// the fp8 x fp8 GEMM of the Fp8Rows route on per-token e4m3 rows -- forward()'s own or the caller's: W8A8 on the policy's e4m3 weights and per-channel scales
        /// (fp8 policy), the per-tensor-scaled form on the resident e4m3 copy (fp4 policy)
        void gemmFp8Rows( uint16_t* y, const uint8_t* x8, const float* ts, int M, int K, int N, void* ws, size_t ws_bytes, mila_stream_t st ) const
        {
            if constexpr ( kFmt == 1 ) rocmCheck( mila_cdna4_gemm_fp8_w8a8_ws( y, x8, static_cast<const uint8_t*>( weight_ ), ts, scales_, bias_, M, K, N, ws, ws_bytes, st ) );
            else rocmCheck( mila_cdna4_gemm_fp8_scaled_ws( y, x8, resident_e4m3_->data(), ts, weight_fp8_scale_->data(), bias_, M, K, N, ws, ws_bytes, st ) );
        }
        /// the test instrument above: copy this call's e4m3 activations and scales to the host when a tap is installed
        void recordTap( const uint8_t* x8, const float* ts, int M, int K, int N ) const
        {
            ActivationTap* tap = activationTap();
            if ( !tap ) return;
            ActivationTap::Record r{ M, K, N, std::vector<uint8_t>( static_cast<size_t>( M ) * K ), std::vector<float>( static_cast<size_t>( M ) ) };
            rocmCheck( mila_cdna4_memcpy_d2h( r.x8.data(), x8, r.x8.size(), this->context_->getStream() ) );
            rocmCheck( mila_cdna4_memcpy_d2h( r.ts.data(), ts, r.ts.size() * 4, this->context_->getStream() ) );
            this->context_->synchronize();
            tap->records.push_back( std::move( r ) );
        }
        /// bytes of the per-token e4m3 activations [M, K] + their scales [M], each rounded up to 16
        static size_t activationBytes( int M, int K ) { return ( ( (size_t)M * K + 15 ) & ~(size_t)15 ) + ( ( (size_t)M * 4 + 15 ) & ~(size_t)15 ); }
        /// scratch for them (+ `extra` bytes behind them, 16-byte aligned: the GEMM's workspace) -- fetched per forward, never cached
        void activationScratch( int M, int K, uint8_t*& x8, float*& ts, size_t extra = 0, void** extra_out = nullptr ) const
        {
            const size_t xb = ( (size_t)M * K + 15 ) & ~(size_t)15, all = activationBytes( M, K );
            auto* base = static_cast<uint8_t*>( this->context_->getScratch( all + extra ) );
            x8 = base; ts = reinterpret_cast<float*>( base + xb );
            if ( extra_out ) *extra_out = extra ? base + all : nullptr;
        }

        void refreshResident()
        {
            if constexpr ( kFmt == 0 ) return;
            if ( !resident_ || !weight_ || !scales_ ) return;
            const int K = narrowToKernelIndex( cfg_.in_features, "in_features" ), N = narrowToKernelIndex( cfg_.out_features, "out_features" );
            mila_stream_t st = this->context_->getStream();
            // the shadows are an optimisation: if the device cannot hold them, fall back to per-forward staging (same results)
            try
            {
                if constexpr ( kFmt == 1 )
                {
                    if ( use_fp8_activation_prefill_ ) return;      // W8A8 reads the policy's own e4m3 weights: nothing to stage
                    if ( !resident_bf16_ ) resident_bf16_ = std::make_unique<RocmBf16Tensor>( this->context_->getDeviceId(), shape_t{ cfg_.out_features, cfg_.in_features } );
                }
                else if constexpr ( kFmt == 2 )
                {
                    if ( !weight_fp8_scale_ || K % 32 != 0 ) return;
                    if ( !resident_e4m3_ ) resident_e4m3_ = std::make_unique<Tensor<TensorDataType::FP8_E4M3, RocmDeviceMemoryResource>>( this->context_->getDeviceId(), shape_t{ cfg_.out_features, cfg_.in_features } );
                }
            }
            catch ( const std::exception& )
            {
                resident_ = false; resident_bf16_.reset(); resident_e4m3_.reset();
                return;
            }
            if constexpr ( kFmt == 1 ) rocmCheck( mila_cdna4_dequantize_to_bf16( resident_bf16_->data(), weight_, scales_, 1, N, K, 0, st ) );
            else if constexpr ( kFmt == 2 )
                rocmCheck( mila_cdna4_upcast_fp4_to_fp8( resident_e4m3_->data(), static_cast<const uint8_t*>( weight_ ), scales_, weight_fp8_scale_->data(), N, K, kGroup, st ) );
        }
    };

    template<typename TPolicy>
    struct OperationTraits<OperationType::LinearOp, DeviceType::Rocm, TensorDataType::BF16, TPolicy>
    {
        using type = RocmLinearOp<TensorDataType::BF16, TPolicy>;
    };
    /// the FP32 validation row: unquantized weights only (OperationTraits.Cuda.ixx:50-54)
    template<>
    struct OperationTraits<OperationType::LinearOp, DeviceType::Rocm, TensorDataType::FP32, Quant::Weight::NoWeightQuant>
    {
        using type = RocmLinearOp<TensorDataType::FP32, Quant::Weight::NoWeightQuant>;
    };
    // PerGroupInt4 has no row, like the quantize path of the reference (CudaLinearOp.ixx:385-391)
    template<int G>
    struct OperationTraits<OperationType::LinearOp, DeviceType::Rocm, TensorDataType::BF16, Quant::Weight::PerGroupInt4<G>>;

    // ---------------------------------------------------------------------------------------
    // RMSNorm / LayerNorm / Softmax / GELU / GeGLU / Residual
    // ---------------------------------------------------------------------------------------
    struct NormOpConfig
    {
        dim_t dim{ 0 };
        float epsilon{ 1e-5f };
        bool has_bias{ true };
        float weight_offset{ 0.0f };   ///< RmsNormConfig unit_offset
    };

    class RocmRmsNormOp : public Operation<DeviceType::Rocm, TensorDataType::BF16>
    {
    public:
        using TensorType = RocmBf16Tensor;
        RocmRmsNormOp( IExecutionContext* ctx, const NormOpConfig& cfg ) : Operation( ctx ), cfg_( cfg )
        {
            if ( cfg.dim <= 0 ) throw std::invalid_argument( "RocmRmsNormOp: normalized dimension must be positive" );
        }
        void setParameters( ITensor* weight, ITensor* bias )
        {
            w_ = weight ? static_cast<const uint16_t*>( weight->rawData() ) : nullptr;
            b_ = bias ? static_cast<const uint16_t*>( bias->rawData() ) : nullptr;
        }
        /// fixes the normalized (trailing) axis and the maximum slice count, and allocates the per-slice rstd the forward pass
        /// writes -- op-owned, bf16 like the reference's (RmsNormOp.ixx:174-262: rstd_tensor_ of num_slices elements)
        void build( const BuildContext& ctx )
        {
            if ( ctx.inputShape().back() != cfg_.dim ) throw std::invalid_argument( "RocmRmsNormOp::build: trailing dimension does not match the normalized shape" );
            const dim_t slices = shapeSize( ctx.inputShape() ) / cfg_.dim;
            rstd_ = std::make_unique<TensorType>( context_->getDeviceId(), shape_t{ slices } );
            built_ = true;
        }
        /// launch geometry follows the runtime tensor (built once at the prefill shape, decode arrives with one row, :271-300)
        void forward( const TensorType& in, TensorType& out ) const
        {
            if ( !built_ ) throw std::runtime_error( "RocmRmsNormOp::forward: not built" );
            if ( in.shape().empty() || in.shape().back() != cfg_.dim ) throw std::runtime_error( "RocmRmsNormOp::forward: input shape is incompatible with the built normalization axis" );
            const int dim = narrowToKernelIndex( cfg_.dim, "dim" );
            const int outer = narrowToKernelIndex( static_cast<dim_t>( in.size() ) / cfg_.dim, "outer" );
            if ( static_cast<size_t>( outer ) > rstd_->size() ) throw std::runtime_error( "RocmRmsNormOp::forward: runtime slice count exceeds the built maximum" );
            rocmCheck( mila_cdna4_rmsnorm_bf16( static_cast<uint16_t*>( out.rawData() ), rstd_->data(), static_cast<const uint16_t*>( in.rawData() ), w_, b_,
                                                outer, 1, dim, cfg_.epsilon, cfg_.weight_offset, context_->getStream() ) );
        }
        /// `outer` rows of caller-owned memory, any count, no rstd kept: the same kernel and bits per row as forward()
        void forwardRows( const uint16_t* in, uint16_t* out, int outer ) const
        {
            rocmCheck( mila_cdna4_rmsnorm_bf16( out, nullptr, in, w_, b_, outer, 1, narrowToKernelIndex( cfg_.dim, "dim" ), cfg_.epsilon, cfg_.weight_offset, context_->getStream() ) );
        }
        const TensorType* rstd() const noexcept { return rstd_.get(); }
        size_t stateBytes() const noexcept { return rstd_ ? rstd_->sizeInBytes() : 0; }
        const uint16_t* weightPtr() const noexcept { return w_; }
        float epsilon() const noexcept { return cfg_.epsilon; }
    private:
        NormOpConfig cfg_;
        const uint16_t* w_{ nullptr };
        const uint16_t* b_{ nullptr };
        std::unique_ptr<TensorType> rstd_;
        bool built_{ false };
    };
    template<> struct OperationTraits<OperationType::RmsNormOp, DeviceType::Rocm, TensorDataType::BF16> { using type = RocmRmsNormOp; };

    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    class RocmLayerNormOp : public Operation<DeviceType::Rocm, TPrecision>
    {
    public:
        using TensorType = RocmTensor<TPrecision>;
        RocmLayerNormOp( IExecutionContext* ctx, const NormOpConfig& cfg ) : Operation<DeviceType::Rocm, TPrecision>( ctx ), cfg_( cfg ) {}
        void setParameters( ITensor* weight, ITensor* bias )
        {
            w_ = weight ? weight->rawData() : nullptr;
            b_ = bias ? bias->rawData() : nullptr;
        }
        void build( const BuildContext& ) { built_ = true; }
        void forward( const TensorType& in, TensorType& out ) const
        {
            if ( !built_ ) throw std::runtime_error( "RocmLayerNormOp::forward: operation must be built before forward()" );
            const int dim = narrowToKernelIndex( cfg_.dim, "dim" );
            const int outer = narrowToKernelIndex( static_cast<dim_t>( in.size() ) / cfg_.dim, "outer" );
            if constexpr ( TPrecision == TensorDataType::FP32 )
                rocmCheck( mila_cdna4_layernorm_fp32( static_cast<float*>( out.rawData() ), nullptr, nullptr, static_cast<const float*>( in.rawData() ), static_cast<const float*>( w_ ),
                                                      static_cast<const float*>( b_ ), outer, dim, cfg_.epsilon, this->context_->getStream() ) );
            else
                rocmCheck( mila_cdna4_layernorm_bf16( static_cast<uint16_t*>( out.rawData() ), nullptr, nullptr, static_cast<const uint16_t*>( in.rawData() ),
                                                      static_cast<const uint16_t*>( w_ ), static_cast<const uint16_t*>( b_ ), outer, dim, cfg_.epsilon, this->context_->getStream() ) );
        }
    private:
        NormOpConfig cfg_;
        const void* w_{ nullptr };
        const void* b_{ nullptr };
        bool built_{ false };
    };
    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    struct OperationTraits<OperationType::LayerNormOp, DeviceType::Rocm, TPrecision> { using type = RocmLayerNormOp<TPrecision>; };

    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    class RocmGeluOp : public Operation<DeviceType::Rocm, TPrecision>
    {
    public:
        using TensorType = RocmTensor<TPrecision>;
        explicit RocmGeluOp( IExecutionContext* ctx ) : Operation<DeviceType::Rocm, TPrecision>( ctx ) {}
        void forward( const TensorType& in, TensorType& out ) const
        {
            if constexpr ( TPrecision == TensorDataType::FP32 )
                rocmCheck( mila_cdna4_gelu_fp32( static_cast<float*>( out.rawData() ), static_cast<const float*>( in.rawData() ), static_cast<int64_t>( in.size() ), this->context_->getStream() ) );
            else
                rocmCheck( mila_cdna4_gelu_bf16( static_cast<uint16_t*>( out.rawData() ), static_cast<const uint16_t*>( in.rawData() ),
                                                 static_cast<int64_t>( in.size() ), this->context_->getStream() ) );
        }
    };
    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    struct OperationTraits<OperationType::GeluOp, DeviceType::Rocm, TPrecision> { using type = RocmGeluOp<TPrecision>; };

    /// Swiglu<..., Gelu> resolves to the GeGLU op (Gemma.Block.ixx:150)
    class RocmGegluOp : public Operation<DeviceType::Rocm, TensorDataType::BF16>
    {
    public:
        using TensorType = RocmBf16Tensor;
        explicit RocmGegluOp( IExecutionContext* ctx ) : Operation( ctx ) {}
        void forward( const TensorType& in, TensorType& out ) const
        {
            const dim_t two_h = in.shape().back();
            if ( two_h % 2 != 0 ) throw std::invalid_argument( "RocmGegluOp::forward: the last dimension must be even ([gate | up])" );
            const int half = narrowToKernelIndex( two_h / 2, "half" );
            const int tokens = narrowToKernelIndex( static_cast<dim_t>( in.size() ) / two_h, "tokens" );
            rocmCheck( mila_cdna4_geglu_bf16( static_cast<uint16_t*>( out.rawData() ), static_cast<const uint16_t*>( in.rawData() ), tokens, half, context_->getStream() ) );
        }
    };
    template<> struct OperationTraits<OperationType::GegluOp, DeviceType::Rocm, TensorDataType::BF16> { using type = RocmGegluOp; };

    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    class RocmResidualOp : public Operation<DeviceType::Rocm, TPrecision>
    {
    public:
        using TensorType = RocmTensor<TPrecision>;
        explicit RocmResidualOp( IExecutionContext* ctx ) : Operation<DeviceType::Rocm, TPrecision>( ctx ) {}
        void forward( const TensorType& a, const TensorType& b, TensorType& out ) const
        {
            if ( a.size() != b.size() ) throw std::invalid_argument( "RocmResidualOp::forward: operand sizes differ" );
            if constexpr ( TPrecision == TensorDataType::FP32 )
                rocmCheck( mila_cdna4_residual_fp32( static_cast<float*>( out.rawData() ), static_cast<const float*>( a.rawData() ), static_cast<const float*>( b.rawData() ),
                                                     static_cast<int64_t>( a.size() ), this->context_->getStream() ) );
            else
                rocmCheck( mila_cdna4_residual_bf16( static_cast<uint16_t*>( out.rawData() ), static_cast<const uint16_t*>( a.rawData() ),
                                                     static_cast<const uint16_t*>( b.rawData() ), static_cast<int64_t>( a.size() ), this->context_->getStream() ) );
        }
    };
    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    struct OperationTraits<OperationType::ResidualOp, DeviceType::Rocm, TPrecision> { using type = RocmResidualOp<TPrecision>; };

    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    class RocmSoftmaxOp : public Operation<DeviceType::Rocm, TPrecision>
    {
    public:
        using TensorType = RocmTensor<TPrecision>;
        RocmSoftmaxOp( IExecutionContext* ctx, int axis ) : Operation<DeviceType::Rocm, TPrecision>( ctx ), axis_( axis ) {}
        void forward( const TensorType& in, TensorType& out ) const
        {
            const auto& s = in.shape();
            const int rank = static_cast<int>( s.size() );
            const int ax = axis_ < 0 ? axis_ + rank : axis_;
            if ( ax < 0 || ax >= rank ) throw std::invalid_argument( "RocmSoftmaxOp::forward: axis out of range" );
            dim_t outer = 1, inner = 1;
            for ( int i = 0; i < ax; ++i ) outer *= s[ i ];
            for ( int i = ax + 1; i < rank; ++i ) inner *= s[ i ];
            if constexpr ( TPrecision == TensorDataType::FP32 )
                rocmCheck( mila_cdna4_softmax_fp32( static_cast<float*>( out.rawData() ), static_cast<const float*>( in.rawData() ), narrowToKernelIndex( outer, "outer" ),
                                                    narrowToKernelIndex( s[ ax ], "dim" ), narrowToKernelIndex( inner, "inner" ), this->context_->getStream() ) );
            else
                rocmCheck( mila_cdna4_softmax_bf16( static_cast<uint16_t*>( out.rawData() ), static_cast<const uint16_t*>( in.rawData() ),
                                                    narrowToKernelIndex( outer, "outer" ), narrowToKernelIndex( s[ ax ], "dim" ),
                                                    narrowToKernelIndex( inner, "inner" ), this->context_->getStream() ) );
        }
    private:
        int axis_;
    };
    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    struct OperationTraits<OperationType::SoftmaxOp, DeviceType::Rocm, TPrecision> { using type = RocmSoftmaxOp<TPrecision>; };

    // ---------------------------------------------------------------------------------------
    // RoPE (IPositionalPairedOp) -- cache built once per (max_seq, head_dim, base, rotary_dim)
    // ---------------------------------------------------------------------------------------
    struct RopeOpConfig
    {
        dim_t max_seq{ 0 }, head_dim{ 0 }, num_heads{ 0 }, num_kv_heads{ 0 };
        float base{ 10000.0f };
        dim_t rotary_dim{ 0 };
    };

    /// Process-wide cos / sin tables, one pair per distinct (device, max_seq, head_dim, base, rotary_dim): every layer of a model that rotates with the same geometry
    /// shares ONE pair (the reference's RopeCacheRegistry, Gemma.ixx:455-462: "only one per distinct key is ever allocated: Gemma has two, the local and global theta").
    /// Entries are weak: the tables live as long as an op holds them.
    class RopeCacheRegistry
    {
    public:
        using CacheTensor = Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>;
        struct Tables { std::shared_ptr<CacheTensor> cos, sin; };
        /// the shared pair for this key; `created` says whether the caller must fill it
        static Tables acquire( DeviceId dev, const std::tuple<int, dim_t, dim_t, uint32_t, dim_t>& key, dim_t max_seq, dim_t head_dim, bool& created )
        {
            static std::mutex mu;
            static std::map<std::tuple<int, dim_t, dim_t, uint32_t, dim_t>, std::pair<std::weak_ptr<CacheTensor>, std::weak_ptr<CacheTensor>>> entries;
            std::lock_guard<std::mutex> lock( mu );
            auto& e = entries[ key ];
            Tables t{ e.first.lock(), e.second.lock() };
            created = !t.cos || !t.sin;
            if ( created )
            {
                t.cos = std::make_shared<CacheTensor>( dev, shape_t{ max_seq, head_dim / 2 } );
                t.sin = std::make_shared<CacheTensor>( dev, shape_t{ max_seq, head_dim / 2 } );
                e = { t.cos, t.sin };
            }
            return t;
        }
    };

    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    class RocmRopeOp : public Operation<DeviceType::Rocm, TPrecision>
    {
        using Operation<DeviceType::Rocm, TPrecision>::context_;
    public:
        using TensorType = RocmTensor<TPrecision>;
        using CacheTensor = Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>;
        RocmRopeOp( IExecutionContext* ctx, const RopeOpConfig& cfg ) : Operation<DeviceType::Rocm, TPrecision>( ctx ), cfg_( cfg )
        {
            if ( cfg.head_dim <= 0 || cfg.head_dim % 2 != 0 ) throw std::invalid_argument( "RocmRopeOp: head_dim must be positive and even" );
            if ( cfg.max_seq <= 0 ) throw std::invalid_argument( "RocmRopeOp: max_seq must be positive" );
        }
        void build( const BuildContext& )
        {
            uint32_t base_bits;
            std::memcpy( &base_bits, &cfg_.base, 4 );
            bool created = false;
            auto t = RopeCacheRegistry::acquire( context_->getDeviceId(), { context_->getDeviceId().index, cfg_.max_seq, cfg_.head_dim, base_bits, cfg_.rotary_dim }, cfg_.max_seq, cfg_.head_dim, created );
            cos_ = t.cos; sin_ = t.sin;
            if ( created )
            {
                rocmCheck( mila_cdna4_rope_build_cache( cos_->data(), sin_->data(), narrowToKernelIndex( cfg_.max_seq, "max_seq" ),
                                                        narrowToKernelIndex( cfg_.head_dim, "head_dim" ), cfg_.base,
                                                        narrowToKernelIndex( cfg_.rotary_dim, "rotary_dim" ), context_->getStream() ) );
                context_->synchronize();      // another op (another context's stream) may read the shared tables next
            }
            built_ = true;
        }
        /// what ONE owner of these tables pays (Rope.ixx:254: the operation reports one owner's bytes; a composite whose layers share a key subtracts the duplicates)
        size_t stateBytes() const noexcept { return ( cos_ ? cos_->sizeInBytes() : 0 ) + ( sin_ ? sin_->sizeInBytes() : 0 ); }
        size_t requiredStateBytes() const noexcept { return 2 * static_cast<size_t>( cfg_.max_seq ) * static_cast<size_t>( cfg_.head_dim / 2 ) * sizeof( float ); }
        const void* tableKey() const noexcept { return cos_.get(); }      ///< equal for ops that share one pair
        /// rotate q [B,T,NH,HS] and k [B,T,NKV,HS] in place (Components/Encodings/Rope/Rope.ixx:107,160-200)
        void prefill( TensorType& q, TensorType& k, int B, int T, int position_offset ) const
        {
            if ( !built_ ) throw std::runtime_error( "RocmRopeOp: not built" );
            if constexpr ( TPrecision == TensorDataType::FP32 )
            {
                auto* qp = static_cast<float*>( q.rawData() );
                auto* kp = static_cast<float*>( k.rawData() );
                rocmCheck( mila_cdna4_rope_forward_fp32( qp, kp, qp, kp, cos_->data(), sin_->data(), B, T, narrowToKernelIndex( cfg_.num_heads, "NH" ),
                                                         narrowToKernelIndex( cfg_.num_kv_heads, "NKV" ), narrowToKernelIndex( cfg_.head_dim, "HS" ),
                                                         position_offset, narrowToKernelIndex( cfg_.max_seq, "max_seq" ), context_->getStream() ) );
            }
            else
            {
                auto* qp = static_cast<uint16_t*>( q.rawData() );
                auto* kp = static_cast<uint16_t*>( k.rawData() );
                rocmCheck( mila_cdna4_rope_forward_bf16( qp, kp, qp, kp, cos_->data(), sin_->data(), B, T, narrowToKernelIndex( cfg_.num_heads, "NH" ),
                                                         narrowToKernelIndex( cfg_.num_kv_heads, "NKV" ), narrowToKernelIndex( cfg_.head_dim, "HS" ),
                                                         position_offset, narrowToKernelIndex( cfg_.max_seq, "max_seq" ), context_->getStream() ) );
            }
        }
        void decode( TensorType& q, TensorType& k, int B, int position ) const { prefill( q, k, B, 1, position ); }
        const float* cosCache() const noexcept { return cos_ ? cos_->data() : nullptr; }
        const float* sinCache() const noexcept { return sin_ ? sin_->data() : nullptr; }
    private:
        RopeOpConfig cfg_;
        std::shared_ptr<CacheTensor> cos_, sin_;
        bool built_{ false };
    };
    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    struct OperationTraits<OperationType::RopeOp, DeviceType::Rocm, TPrecision> { using type = RocmRopeOp<TPrecision>; };

    // ---------------------------------------------------------------------------------------
    // Grouped-query attention over an op-owned KV cache (IKvInference)
    // ---------------------------------------------------------------------------------------
    struct GqaOpConfig
    {
        dim_t num_heads{ 0 }, num_kv_heads{ 0 }, head_dim{ 0 };
        dim_t window{ 0 };               ///< 0 = global
        float attention_scale{ 0.0f };   ///< <= 0 -> 1/sqrt(head_dim)  (GroupedQueryAttention.Config.ixx:190-200)
    };

    /// Shared body of the two KV-cache policies of CudaGqaOp<Prec, kBounded> (OPS/Attention/GQA/CudaGqaOp.ixx:97-985): the
    /// policy only changes the cache capacity rule and what rewind may restore, so a model can hold bounded (sliding-window)
    /// and unbounded (global) layers behind one pointer type.
    class RocmGqaOpBase : public Operation<DeviceType::Rocm, TensorDataType::BF16>
    {
    public:
        using TensorType = RocmBf16Tensor;
        RocmGqaOpBase( IExecutionContext* ctx, const GqaOpConfig& cfg, bool bounded_ring ) : Operation( ctx ), cfg_( cfg ), kBoundedRing( bounded_ring )
        {
            if ( cfg.num_heads <= 0 || cfg.num_kv_heads <= 0 || cfg.num_heads % cfg.num_kv_heads != 0 )
                throw std::invalid_argument( "RocmGqaOp: num_heads must be a positive multiple of num_kv_heads" );
            if ( cfg.head_dim <= 0 ) throw std::invalid_argument( "RocmGqaOp: head_dim must be positive" );
            if ( kBoundedRing && cfg.window <= 0 ) throw std::invalid_argument( "RocmGqaOp: a bounded ring cache needs a sliding window" );
        }
        virtual ~RocmGqaOpBase() = default;
        bool boundedRing() const noexcept { return kBoundedRing; }

        float scale() const noexcept { return cfg_.attention_scale > 0.0f ? cfg_.attention_scale : 1.0f / std::sqrt( static_cast<float>( cfg_.head_dim ) ); }

        /// capacity rule of CudaGqaOp::resolveCacheCapacity (CudaGqaOp.ixx:552-574)
        dim_t resolveCacheCapacity( dim_t max_seq, dim_t window, dim_t prefill_chunk ) const
        {
            if ( kBoundedRing ) return std::min( max_seq, window + std::max<dim_t>( prefill_chunk, 1 ) - 1 );
            return max_seq;
        }

        void initializeKvCache( int batch, dim_t max_seq, dim_t prefill_chunk )
        {
            batch_ = batch;
            capacity_ = resolveCacheCapacity( max_seq, cfg_.window, prefill_chunk );
            const shape_t s{ batch, cfg_.num_kv_heads, capacity_, cfg_.head_dim };
            k_cache_ = std::make_unique<TensorType>( context_->getDeviceId(), s );
            v_cache_ = std::make_unique<TensorType>( context_->getDeviceId(), s );
            length_ = 0;
            rows_ = 1; row_ = 0;
        }
        /// Batched decode of independent sequences: `rows` caches [rows, NKV, capacity, HS] behind this B = 1 op, one per sequence.  selectCacheRow( b ) makes row b
        /// the cache every B = 1 call of this op (prefill, decode, keyCache() / valueCache()) works on, so the existing prefill writes row b unchanged; the rows decode
        /// entry takes keyCacheRows() / valueCacheRows(), all rows.  Call after initializeKvCache(); rows == 1 leaves the op as it was built.
        void setCacheRows( int rows )
        {
            requireCache();
            if ( rows < 1 ) throw std::invalid_argument( "RocmGqaOp::setCacheRows: rows must be positive" );
            if ( rows == rows_ ) return;
            const shape_t s{ rows, cfg_.num_kv_heads, capacity_, cfg_.head_dim };
            k_cache_ = std::make_unique<TensorType>( context_->getDeviceId(), s );
            v_cache_ = std::make_unique<TensorType>( context_->getDeviceId(), s );
            rows_ = rows; row_ = 0; length_ = 0;
        }
        void selectCacheRow( int b )
        {
            if ( b < 0 || b >= rows_ ) throw std::invalid_argument( "RocmGqaOp::selectCacheRow: row " + std::to_string( b ) + " outside the " + std::to_string( rows_ ) + " cache rows" );
            row_ = b;
        }
        int cacheRows() const noexcept { return rows_; }
        uint16_t* keyCacheRows() noexcept { return k_cache_ ? k_cache_->data() : nullptr; }
        uint16_t* valueCacheRows() noexcept { return v_cache_ ? v_cache_->data() : nullptr; }
        void resetKvCache() noexcept { length_ = 0; }
        void rewindKvCache( dim_t length )
        {
            if ( length < 0 || length > length_ ) throw std::invalid_argument( "RocmGqaOp::rewindKvCache: bad length" );
            // ring validity as the reference states it (CudaGqaOp.ixx:182-203): a continuation from `length` attends down to length - window,
            // so the stale tail [length, length_) must not have wrapped over that range: at most capacity - window (= chunk - 1) stale tokens
            if ( kBoundedRing && length_ - length > capacity_ - cfg_.window ) throw std::runtime_error( "RocmGqaOp::rewindKvCache: evicted positions cannot be restored" );
            length_ = length;
        }
        dim_t cacheLength() const noexcept { return length_; }
        /// a caller that appended through the fused entry points (which take the cache pointers directly) reports how far it wrote
        void noteCacheLength( dim_t length ) { if ( length < 0 ) throw std::invalid_argument( "RocmGqaOp::noteCacheLength: negative length" ); length_ = length; }
        dim_t cacheCapacity() const noexcept { return capacity_; }

        /// q [B,chunk,NH*HS], k/v [B,chunk,NKV*HS] at absolute positions [position, position+chunk)
        void prefill( const TensorType& q, const TensorType& k, const TensorType& v, TensorType& out, int chunk, int position )
        {
            requireCache();
            mila_stream_t st = context_->getStream();
            const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            rocmCheck( mila_cdna4_kv_write_bf16( keyCache(), valueCache(), q_cast( k ), q_cast( v ), batch_, chunk, NKV, HS, position, cap, st ) );
            rocmCheck( mila_cdna4_attn_prefill_bf16( out.data(), q_cast( q ), keyCache(), valueCache(), batch_, chunk, NH, NKV, HS, cap,
                                                     position, (int)cfg_.window, scale(), st ) );
            length_ = position + chunk;
        }

        /// the chunk's K/V rows are already in the cache (written by the fused q/k/v post-processing kernel):
        /// attention only.  q [B,chunk,NH*HS] at absolute positions [position, position+chunk)
        void prefillFromCache( const TensorType& q, TensorType& out, int chunk, int position )
        {
            requireCache();
            const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            rocmCheck( mila_cdna4_attn_prefill_bf16( out.data(), q_cast( q ), keyCache(), valueCache(), batch_, chunk, NH, NKV, HS, cap,
                                                     position, (int)cfg_.window, scale(), context_->getStream() ) );
            length_ = position + chunk;
        }

        /// one token per sequence at absolute position `position`
        void decode( const TensorType& q, const TensorType& k, const TensorType& v, TensorType& out, int position )
        {
            requireCache();
            mila_stream_t st = context_->getStream();
            const int NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            rocmCheck( mila_cdna4_kv_write_bf16( keyCache(), valueCache(), q_cast( k ), q_cast( v ), batch_, 1, NKV, HS, position, cap, st ) );
            attendDecode( q, out, position );
        }

        /// attention only (the fused q/k/v post-processing kernel has already appended K/V)
        void attendDecode( const TensorType& q, TensorType& out, int position )
        {
            requireCache();
            const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            const size_t need = mila_cdna4_attn_decode_scratch_bytes( batch_, NH, HS );
            void* scratch = context_->getScratch( need );   // fetched per forward, never cached
            rocmCheck( mila_cdna4_attn_decode_bf16( out.data(), q_cast( q ), keyCache(), valueCache(), scratch, need, batch_, NH, NKV, HS, cap,
                                                    position + 1, (int)cfg_.window, scale(), context_->getStream() ) );
            length_ = position + 1;
        }

        size_t stateBytes() const noexcept { return ( k_cache_ ? k_cache_->sizeInBytes() : 0 ) + ( v_cache_ ? v_cache_->sizeInBytes() : 0 ); }
        size_t requiredStateBytes( int batch, dim_t max_seq, dim_t prefill_chunk ) const
        {
            return 2 * static_cast<size_t>( batch ) * static_cast<size_t>( cfg_.num_kv_heads ) * static_cast<size_t>( resolveCacheCapacity( max_seq, cfg_.window, prefill_chunk ) ) *
                   static_cast<size_t>( cfg_.head_dim ) * 2;
        }
        /// the selected row's caches (row 0 unless selectCacheRow() said otherwise)
        uint16_t* keyCache() noexcept { return k_cache_ ? k_cache_->data() + rowElems() * static_cast<size_t>( row_ ) : nullptr; }
        uint16_t* valueCache() noexcept { return v_cache_ ? v_cache_->data() + rowElems() * static_cast<size_t>( row_ ) : nullptr; }
        const GqaOpConfig& config() const noexcept { return cfg_; }

    private:
        static const uint16_t* q_cast( const TensorType& t ) { return static_cast<const uint16_t*>( t.rawData() ); }
        void requireCache() const { if ( !k_cache_ ) throw std::runtime_error( "RocmGqaOp: initializeKvCache() must be called first" ); }
        GqaOpConfig cfg_;
        const bool kBoundedRing;
        std::unique_ptr<TensorType> k_cache_, v_cache_;
        size_t rowElems() const noexcept { return static_cast<size_t>( batch_ ) * static_cast<size_t>( cfg_.num_kv_heads ) * static_cast<size_t>( capacity_ ) * static_cast<size_t>( cfg_.head_dim ); }
        int batch_{ 1 };
        int rows_{ 1 }, row_{ 0 };      ///< independent caches behind the op, and the one its B = 1 calls work on
        dim_t capacity_{ 0 }, length_{ 0 };
    };
    /// counterpart of CudaGqaOp<Prec, kBounded>: the KV policy as a compile-time axis, as in the reference
    template<bool kBoundedRingPolicy>
    class RocmGqaOp : public RocmGqaOpBase
    {
    public:
        RocmGqaOp( IExecutionContext* ctx, const GqaOpConfig& cfg ) : RocmGqaOpBase( ctx, cfg, kBoundedRingPolicy ) {}
    };
    template<typename TKvPolicy>
    struct OperationTraits<OperationType::GroupedQueryAttentionOp, DeviceType::Rocm, TensorDataType::BF16, TKvPolicy>
    {
        using type = RocmGqaOp<TKvPolicy::kBoundedRing>;
    };

    /// The op row of Quant::KvCache::PerChannelKvFp8<> (Quantization/KvCache/QuantPolicy.ixx:56-88; the reference's BACKLOG names the row
    /// OperationTraits<GqaOp, Cuda, BF16, PerChannelKvFp8<>> and has no kernels for it): the public methods of RocmGqaOpBase over an op-owned e4m3 cache with one
    /// fp32 scale per KV head per cached token (csrc/attention_kvfp8.hip).  The cache is unbounded: capacity = max_seq.  Queries, outputs and the appended K / V
    /// rows stay BF16; a cached value is read back as bf16( e4m3 * scale ) -- by the decode kernels in registers (on the way into LDS in the matrix-core form a 16-head
    /// group takes from the 8192-key bucket on), in a transient bf16 cache by the prefill.
    class RocmGqaKvFp8Op : public Operation<DeviceType::Rocm, TensorDataType::BF16>
    {
    public:
        using TensorType = RocmBf16Tensor;
        using StorageTensor = RocmTensor<TensorDataType::FP8_E4M3>;
        using ScaleTensor = RocmTensor<TensorDataType::FP32>;
        RocmGqaKvFp8Op( IExecutionContext* ctx, const GqaOpConfig& cfg ) : Operation( ctx ), cfg_( cfg )
        {
            if ( cfg.num_heads <= 0 || cfg.num_kv_heads <= 0 || cfg.num_heads % cfg.num_kv_heads != 0 )
                throw std::invalid_argument( "RocmGqaKvFp8Op: num_heads must be a positive multiple of num_kv_heads" );
            if ( cfg.head_dim != 64 && cfg.head_dim != 128 && cfg.head_dim != 256 && cfg.head_dim != 512 )
                throw std::invalid_argument( "RocmGqaKvFp8Op: head_dim must be 64, 128, 256 or 512" );
            if ( cfg.window < 0 ) throw std::invalid_argument( "RocmGqaKvFp8Op: window must be >= 0" );
        }
        bool boundedRing() const noexcept { return false; }
        float scale() const noexcept { return cfg_.attention_scale > 0.0f ? cfg_.attention_scale : 1.0f / std::sqrt( static_cast<float>( cfg_.head_dim ) ); }
        dim_t resolveCacheCapacity( dim_t max_seq, dim_t /*window*/, dim_t /*prefill_chunk*/ ) const { return max_seq; }

        /// four tensors: K8 / V8 [B, NKV, capacity, HS] e4m3, Ks / Vs [B, NKV, capacity] fp32
        void initializeKvCache( int batch, dim_t max_seq, dim_t /*prefill_chunk*/ )
        {
            batch_ = batch;
            capacity_ = max_seq;
            const shape_t s8{ batch, cfg_.num_kv_heads, capacity_, cfg_.head_dim }, ss{ batch, cfg_.num_kv_heads, capacity_ };
            k8_ = std::make_unique<StorageTensor>( context_->getDeviceId(), s8 );
            v8_ = std::make_unique<StorageTensor>( context_->getDeviceId(), s8 );
            ks_ = std::make_unique<ScaleTensor>( context_->getDeviceId(), ss );
            vs_ = std::make_unique<ScaleTensor>( context_->getDeviceId(), ss );
            length_ = 0;
            rows_ = 1; row_ = 0;
        }
        /// Batched decode of independent sequences, as RocmGqaOp::setCacheRows: `rows` caches [rows, NKV, capacity(, HS)] behind this B = 1 op, one per sequence.
        /// selectCacheRow( b ) makes row b the cache every B = 1 call of this op (prefill, attendPrefill, decode*, keyBytes() and its siblings) works on, so the
        /// existing prefill and the fused prefill append write row b unchanged; the rows entries (fused_qkv_post_kvfp8_rows_devpos, attn_decode_kvfp8_rows,
        /// kv_rows_fork_layers_kvfp8) take keyBytesRows() and its siblings, all rows.  Call after initializeKvCache(); rows == 1 leaves the op as it was built.
        void setCacheRows( int rows )
        {
            requireCache();
            if ( rows < 1 ) throw std::invalid_argument( "RocmGqaKvFp8Op::setCacheRows: rows must be positive" );
            if ( rows == rows_ ) return;
            const shape_t s8{ rows, cfg_.num_kv_heads, capacity_, cfg_.head_dim }, ss{ rows, cfg_.num_kv_heads, capacity_ };
            k8_ = std::make_unique<StorageTensor>( context_->getDeviceId(), s8 );
            v8_ = std::make_unique<StorageTensor>( context_->getDeviceId(), s8 );
            ks_ = std::make_unique<ScaleTensor>( context_->getDeviceId(), ss );
            vs_ = std::make_unique<ScaleTensor>( context_->getDeviceId(), ss );
            rows_ = rows; row_ = 0; length_ = 0;
        }
        void selectCacheRow( int b )
        {
            if ( b < 0 || b >= rows_ ) throw std::invalid_argument( "RocmGqaKvFp8Op::selectCacheRow: row " + std::to_string( b ) + " outside the " + std::to_string( rows_ ) + " cache rows" );
            row_ = b;
        }
        int cacheRows() const noexcept { return rows_; }
        void resetKvCache() noexcept { length_ = 0; }
        void rewindKvCache( dim_t length )
        {
            if ( length < 0 || length > length_ ) throw std::invalid_argument( "RocmGqaKvFp8Op::rewindKvCache: bad length" );
            length_ = length;      // unbounded: every earlier row is still there, and a row's bytes and scale do not depend on later rows
        }
        dim_t cacheLength() const noexcept { return length_; }
        /// a caller that appended through decodeAt() (whose position lives on the device) reports how far it wrote
        void noteCacheLength( dim_t length )
        {
            if ( length < 0 || length > capacity_ ) throw std::invalid_argument( "RocmGqaKvFp8Op::noteCacheLength: length outside [0, capacity]" );
            length_ = length;
        }
        dim_t cacheCapacity() const noexcept { return capacity_; }

        /// q [B,chunk,NH*HS], k/v [B,chunk,NKV*HS] at absolute positions [position, position+chunk): quantizing append, then the bf16 flash prefill on the band
        /// dequantized into the context's scratch
        void prefill( const TensorType& q, const TensorType& k, const TensorType& v, TensorType& out, int chunk, int position )
        {
            requireCache();
            mila_stream_t st = context_->getStream();
            const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            rocmCheck( mila_cdna4_kv_write_fp8( keyBytes(), valueBytes(), keyScaleData(), valueScaleData(), q_cast( k ), q_cast( v ), batch_, chunk, NKV, HS, position, cap, st ) );
            const size_t need = mila_cdna4_attn_prefill_kvfp8_scratch_bytes( batch_, NKV, HS, cap );
            void* scratch = context_->getScratch( need );   // fetched per call, never cached
            rocmCheck( mila_cdna4_attn_prefill_kvfp8( out.data(), q_cast( q ), keyBytes(), valueBytes(), keyScaleData(), valueScaleData(), scratch, need, batch_, chunk, NH, NKV, HS,
                                                      cap, position, (int)cfg_.window, scale(), st ) );
            length_ = position + chunk;
        }
        /// one token per sequence at absolute position `position`
        void decode( const TensorType& q, const TensorType& k, const TensorType& v, TensorType& out, int position )
        {
            requireCache();
            const int NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            rocmCheck( mila_cdna4_kv_write_fp8( keyBytes(), valueBytes(), keyScaleData(), valueScaleData(), q_cast( k ), q_cast( v ), batch_, 1, NKV, HS, position, cap,
                                                context_->getStream() ) );
            attendDecode( q, out, position );
        }
        /// attention only, over rows that are already in the cache
        void attendDecode( const TensorType& q, TensorType& out, int position )
        {
            requireCache();
            const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            const size_t need = mila_cdna4_attn_decode_scratch_bytes( batch_, NH, HS );
            void* scratch = context_->getScratch( need );   // fetched per call, never cached
            rocmCheck( mila_cdna4_attn_decode_kvfp8( out.data(), q_cast( q ), keyBytes(), valueBytes(), keyScaleData(), valueScaleData(), scratch, need, batch_, NH, NKV, HS, cap,
                                                     position + 1, (int)cfg_.window, scale(), context_->getStream() ) );
            length_ = position + 1;
        }

        /// decode() with the position in DEVICE memory (graph replay: one captured launch sequence serves every step): appends the token at row *position_dev and
        /// attends over *position_dev + 1 keys.  max_len: an upper bound of the live length inside its band bucket (mila_cdna4_attn_decode_band_bucket), which fixes
        /// the kernel form and split count -- any bound of the bucket gives decode()'s bits.  The op cannot see the device value: cacheLength() is unchanged, the
        /// caller follows up with noteCacheLength( position + 1 ) once it knows the position on the host.
        void decodeAt( const TensorType& q, const TensorType& k, const TensorType& v, TensorType& out, const int32_t* position_dev, int max_len )
        {
            requireCache();
            if ( !position_dev ) throw std::invalid_argument( "RocmGqaKvFp8Op::decodeAt: null device position" );
            mila_stream_t st = context_->getStream();
            const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            rocmCheck( mila_cdna4_kv_write_fp8_devpos( keyBytes(), valueBytes(), keyScaleData(), valueScaleData(), q_cast( k ), q_cast( v ), batch_, NKV, HS, position_dev, cap, st ) );
            const size_t need = mila_cdna4_attn_decode_scratch_bytes( batch_, NH, HS );
            void* scratch = context_->getScratch( need );   // fetched per call, never cached
            rocmCheck( mila_cdna4_attn_decode_kvfp8_devpos( out.data(), q_cast( q ), keyBytes(), valueBytes(), keyScaleData(), valueScaleData(), scratch, need, batch_, NH, NKV, HS, cap,
                                                            position_dev, max_len, (int)cfg_.window, scale(), st ) );
        }

        /// attention only, over rows the quantizing fused append (fused_qkv_post_kvfp8_prefill) has already written: q [B,chunk,NH*HS] at absolute positions
        /// [position, position+chunk); the band is dequantized into the context's scratch, then the bf16 flash prefill runs on it
        void attendPrefill( const TensorType& q, TensorType& out, int chunk, int position )
        {
            requireCache();
            const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            const size_t need = mila_cdna4_attn_prefill_kvfp8_scratch_bytes( batch_, NKV, HS, cap );
            void* scratch = context_->getScratch( need );   // fetched per call, never cached
            rocmCheck( mila_cdna4_attn_prefill_kvfp8( out.data(), q_cast( q ), keyBytes(), valueBytes(), keyScaleData(), valueScaleData(), scratch, need, batch_, chunk, NH, NKV, HS,
                                                      cap, position, (int)cfg_.window, scale(), context_->getStream() ) );
            length_ = position + chunk;
        }
        /// attendDecode() at the position held in device memory: attention over *position_dev + 1 keys, rows already appended (fused_qkv_post_kvfp8_devpos); max_len as
        /// in decodeAt().  cacheLength() is unchanged: noteCacheLength( position + 1 ) once the host knows the position
        void attendDecodeAt( const TensorType& q, TensorType& out, const int32_t* position_dev, int max_len )
        {
            requireCache();
            if ( !position_dev ) throw std::invalid_argument( "RocmGqaKvFp8Op::attendDecodeAt: null device position" );
            const int NH = (int)cfg_.num_heads, NKV = (int)cfg_.num_kv_heads, HS = (int)cfg_.head_dim, cap = (int)capacity_;
            const size_t need = mila_cdna4_attn_decode_scratch_bytes( batch_, NH, HS );
            void* scratch = context_->getScratch( need );   // fetched per call, never cached
            rocmCheck( mila_cdna4_attn_decode_kvfp8_devpos( out.data(), q_cast( q ), keyBytes(), valueBytes(), keyScaleData(), valueScaleData(), scratch, need, batch_, NH, NKV, HS, cap,
                                                            position_dev, max_len, (int)cfg_.window, scale(), context_->getStream() ) );
        }

        /// these three exist for the fused q/k/v post-processing entries (fused_qkv_post, fused_attn_decode), which write a bf16 cache through raw pointers
        void prefillFromCache( const TensorType&, TensorType&, int, int ) { throw std::logic_error( "RocmGqaKvFp8Op::prefillFromCache: " + std::string( kFusedOnly ) ); }
        uint16_t* keyCache() { throw std::logic_error( "RocmGqaKvFp8Op::keyCache: " + std::string( kFusedOnly ) ); }
        uint16_t* valueCache() { throw std::logic_error( "RocmGqaKvFp8Op::valueCache: " + std::string( kFusedOnly ) ); }

        /// 2 * rows * B * NKV * capacity * (HS + 4): one byte per element and one fp32 scale per cached token, K and V
        size_t stateBytes() const noexcept { return tensorBytes( k8_ ) + tensorBytes( v8_ ) + tensorBytes( ks_ ) + tensorBytes( vs_ ); }
        /// (times the cache rows setCacheRows() asked for)
        size_t requiredStateBytes( int batch, dim_t max_seq, dim_t /*prefill_chunk*/ ) const
        {
            return 2 * static_cast<size_t>( rows_ ) * static_cast<size_t>( batch ) * static_cast<size_t>( cfg_.num_kv_heads ) * static_cast<size_t>( max_seq ) * ( static_cast<size_t>( cfg_.head_dim ) + 4 );
        }
        /// the cache arrays (tests read them back): e4m3 bytes and fp32 scales, all rows
        const StorageTensor* keyStorage() const noexcept { return k8_.get(); }
        const StorageTensor* valueStorage() const noexcept { return v8_.get(); }
        const ScaleTensor* keyScales() const noexcept { return ks_.get(); }
        const ScaleTensor* valueScales() const noexcept { return vs_.get(); }
        /// where the selected row's slice starts in them: elements of the byte tensors | of the scale tensors (0 unless selectCacheRow() said otherwise)
        size_t selectedRowByteOffset() const noexcept { return rowScales() * static_cast<size_t>( cfg_.head_dim ) * static_cast<size_t>( row_ ); }
        size_t selectedRowScaleOffset() const noexcept { return rowScales() * static_cast<size_t>( row_ ); }
        /// ... and the selected row's device arrays, for the quantizing fused entries (fused_qkv_post_kvfp8*), which append through raw pointers; null before initializeKvCache()
        uint8_t* keyBytes() noexcept { return k8_ ? keyBytesRows() + selectedRowByteOffset() : nullptr; }
        uint8_t* valueBytes() noexcept { return v8_ ? valueBytesRows() + selectedRowByteOffset() : nullptr; }
        float* keyScaleData() noexcept { return ks_ ? keyScaleDataRows() + selectedRowScaleOffset() : nullptr; }
        float* valueScaleData() noexcept { return vs_ ? valueScaleDataRows() + selectedRowScaleOffset() : nullptr; }
        /// all rows: what the rows entries take
        uint8_t* keyBytesRows() noexcept { return k8_ ? static_cast<uint8_t*>( k8_->rawData() ) : nullptr; }
        uint8_t* valueBytesRows() noexcept { return v8_ ? static_cast<uint8_t*>( v8_->rawData() ) : nullptr; }
        float* keyScaleDataRows() noexcept { return ks_ ? ks_->data() : nullptr; }
        float* valueScaleDataRows() noexcept { return vs_ ? vs_->data() : nullptr; }
        const GqaOpConfig& config() const noexcept { return cfg_; }

    private:
        static constexpr const char* kFusedOnly = "the fused q/k/v entries write a bf16 cache; the FP8 KV cache is appended to by prefill() / decode() only";
        static const uint16_t* q_cast( const TensorType& t ) { return static_cast<const uint16_t*>( t.rawData() ); }
        void requireCache() const { if ( !k8_ ) throw std::runtime_error( "RocmGqaKvFp8Op: initializeKvCache() must be called first" ); }
        GqaOpConfig cfg_;
        std::unique_ptr<StorageTensor> k8_, v8_;
        std::unique_ptr<ScaleTensor> ks_, vs_;
        /// scales (= cached K or V rows) of one cache row
        size_t rowScales() const noexcept { return static_cast<size_t>( batch_ ) * static_cast<size_t>( cfg_.num_kv_heads ) * static_cast<size_t>( capacity_ ); }
        int batch_{ 1 };
        int rows_{ 1 }, row_{ 0 };      ///< independent caches behind the op, and the one its B = 1 calls work on
        dim_t capacity_{ 0 }, length_{ 0 };
    };
    /// more specialised than the TKvPolicy row above; storage other than OCP e4m3 has no kernels
    template<TensorDataType TStorage>
    struct OperationTraits<OperationType::GroupedQueryAttentionOp, DeviceType::Rocm, TensorDataType::BF16, Quant::KvCache::PerChannelKvFp8<TStorage>>
    {
        static_assert( TStorage == TensorDataType::FP8_E4M3,
                       "PerChannelKvFp8: the CDNA4 KV-cache kernels store OCP e4m3 (FP8_E4M3); FP8_E5M2 storage has no GroupedQueryAttentionOp row" );
        using type = RocmGqaKvFp8Op;
    };

    // ---------------------------------------------------------------------------------------
    // Sampling (row f3): counterpart of CudaSamplingOp<FP32> (OPS/Sampling/CudaSamplingOp.ixx; Tests/Dnn/Samplers/Sampling.Cuda.cpp:40-150).
    // forward(): sample on the context's stream into a device token.  enqueueForward() / awaitToken(): the decode-ahead half of the pipelined generation loop --
    // the token is ALSO published to a host-visible slot by the sampler's stream (no host synchronize between forward and sample), awaitToken() blocks until it is
    // there; awaitToken() without an outstanding enqueueForward() is a caller bug: std::logic_error, not UB (Sampling.Cuda.cpp:503-509).
    // ---------------------------------------------------------------------------------------
    struct SamplingOpConfig { dim_t vocab_size{ 0 }; float final_logit_softcap{ 0.0f }; };
    /// Components/Transformers/SamplingParams.ixx: temperature <= 0 = greedy.  The four filters (Specifications/TokenSampling.md 3.3; mila_cdna4.h: sampling filters) are
    /// neutral by default: min_p in [0, 1), repetition_penalty > 0 (1 = off), presence / frequency penalties (0 = off)
    struct SamplingParams
    {
        float temperature{ 1.0f }; int top_k{ 0 }; float top_p{ 1.0f };
        float min_p{ 0.0f }; float repetition_penalty{ 1.0f }; float presence_penalty{ 0.0f }; float frequency_penalty{ 0.0f };
        /// any penalty set: the sampler reads and updates a token table
        bool penalized() const noexcept { return repetition_penalty != 1.0f || presence_penalty != 0.0f || frequency_penalty != 0.0f; }
        bool filtered() const noexcept { return penalized() || min_p != 0.0f; }
        mila_sample_filters filters() const noexcept { return mila_sample_filters{ min_p, repetition_penalty, presence_penalty, frequency_penalty }; }
        /// std::invalid_argument for what the device library refuses: a non-finite value, repetition_penalty <= 0, min_p outside [0, 1)
        void checkFilters( const char* who ) const
        {
            if ( !std::isfinite( min_p ) || !std::isfinite( repetition_penalty ) || !std::isfinite( presence_penalty ) || !std::isfinite( frequency_penalty ) )
                throw std::invalid_argument( std::string( who ) + ": a sampling filter is not finite" );
            if ( !( repetition_penalty > 0.0f ) ) throw std::invalid_argument( std::string( who ) + ": repetition_penalty must be > 0" );
            if ( !( min_p >= 0.0f && min_p < 1.0f ) ) throw std::invalid_argument( std::string( who ) + ": min_p outside [0, 1)" );
        }
    };

    /// The token tables of 1 .. max_rows sequences (mila_cdna4.h: sampling filters -- `vocab` 32-bit words per row: bit 31 = the token occurs in the prompt, bits
    /// 0 .. 30 = the times it has been generated).  The filtered samplers read row b's table beside the logits and count the token they choose; reset() starts a
    /// request.  Everything runs on the context's stream; nothing synchronizes but read().
    class RocmTokenTable
    {
    public:
        RocmTokenTable( IExecutionContext* ctx, dim_t vocab, int max_rows ) : context_( cast_context<DeviceType::Rocm>( ctx ) ), vocab_( vocab ), rows_( max_rows )
        {
            if ( vocab <= 0 || max_rows < 1 ) throw std::invalid_argument( "RocmTokenTable: need a positive vocabulary and at least one row" );
            (void)narrowToKernelIndex( vocab, "vocab" );
            const auto dev = context_->getDeviceId();
            table_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( max_rows ), vocab } );
            stage_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( kStage ) } );
            for ( int b = 0; b < max_rows; ++b ) clear( b );
        }
        uint32_t* data() { return reinterpret_cast<uint32_t*>( table_->data() ); }
        uint32_t* row( int b ) { checkRow( b ); return data() + static_cast<size_t>( b ) * stride(); }
        size_t stride() const noexcept { return static_cast<size_t>( vocab_ ); }
        int rows() const noexcept { return rows_; }
        void clear( int b )
        {
            checkRow( b );
            rocmCheck( mila_cdna4_token_table_clear( data(), stride(), b, static_cast<int>( vocab_ ), context_->getStream() ) );
        }
        /// a new request on row b: every count to zero, the flag of every prompt token set.  The ids travel through a small device staging buffer in stream order.
        void reset( int b, const int32_t* prompt_host, size_t n )
        {
            clear( b );
            for ( size_t i0 = 0; i0 < n; i0 += kStage )
            {
                const size_t c = std::min<size_t>( kStage, n - i0 );
                rocmCheck( mila_cdna4_memcpy_h2d( stage_->data(), prompt_host + i0, c * 4, context_->getStream() ) );
                rocmCheck( mila_cdna4_token_table_mark_prompt( data(), stride(), b, static_cast<int>( vocab_ ), stage_->data(), static_cast<int>( c ), context_->getStream() ) );
            }
        }
        /// row b to the host (synchronizes)
        void read( int b, uint32_t* out )
        {
            rocmCheck( mila_cdna4_memcpy_d2h( out, row( b ), stride() * 4, context_->getStream() ) );
            context_->synchronize();
        }
        size_t stateBytes() const { return table_->sizeInBytes() + stage_->sizeInBytes(); }
        static size_t requiredBytes( dim_t vocab, int max_rows ) { return ( static_cast<size_t>( max_rows ) * static_cast<size_t>( vocab ) + kStage ) * 4; }
    private:
        static constexpr size_t kStage = 1024;
        void checkRow( int b ) const { if ( b < 0 || b >= rows_ ) throw std::invalid_argument( "RocmTokenTable: row " + std::to_string( b ) + " outside 0 .. " + std::to_string( rows_ - 1 ) ); }
        ExecutionContext<DeviceType::Rocm>* context_;
        dim_t vocab_;
        int rows_;
        std::unique_ptr<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>> table_, stage_;
    };

    /// One bias table row (mila_cdna4.h: logit bias -- `vocab` fp32 values, finite or -inf, that the biased samplers add to the capped logit) plus a staging buffer.
    /// The table's address never changes, so a captured step that reads it sees every later update.  Everything runs on the context's stream.  apply() / update()
    /// upload through the staging buffer and return once the ids are consumed (they synchronize); stage() uploads a list ahead of time and commit() enqueues it
    /// later as one small launch without touching the host again -- what a decode-ahead loop puts between two replays.
    class RocmTokenBias
    {
    public:
        RocmTokenBias( IExecutionContext* ctx, dim_t vocab ) : context_( cast_context<DeviceType::Rocm>( ctx ) ), vocab_( vocab )
        {
            if ( vocab <= 0 ) throw std::invalid_argument( "RocmTokenBias: need a positive vocabulary" );
            (void)narrowToKernelIndex( vocab, "vocab" );
            const auto dev = context_->getDeviceId();
            table_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ vocab } );
            stage_ids_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( 2 * kStage ) } );
            stage_values_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( 2 * kStage ) } );
            rocmCheck( mila_cdna4_token_bias_fill( data(), 0, 0, static_cast<int>( vocab_ ), 0.0f, context_->getStream() ) );
        }
        float* data() { return table_->data(); }
        dim_t vocab() const noexcept { return vocab_; }
        /// the whole table: every value `fill`, then values[j] at ids[j]
        void apply( float fill, const int32_t* ids_host, const float* values_host, size_t n )
        {
            rocmCheck( mila_cdna4_token_bias_fill( data(), 0, 0, static_cast<int>( vocab_ ), fill, context_->getStream() ) );
            update( ids_host, values_host, n );
        }
        /// values[j] at ids[j]; the other entries stay
        void update( const int32_t* ids_host, const float* values_host, size_t n )
        {
            for ( size_t i0 = 0; i0 < n; i0 += kStage )
            {
                const size_t c = std::min<size_t>( kStage, n - i0 );
                rocmCheck( mila_cdna4_memcpy_h2d( stage_ids_->data(), ids_host + i0, c * 4, context_->getStream() ) );
                rocmCheck( mila_cdna4_memcpy_h2d( stage_values_->data(), values_host + i0, c * 4, context_->getStream() ) );
                rocmCheck( mila_cdna4_token_bias_set( data(), 0, 0, static_cast<int>( vocab_ ), stage_ids_->data(), stage_values_->data(), static_cast<int>( c ), context_->getStream() ) );
            }
            context_->synchronize();
        }
        /// upload an update of at most kStage entries into the second half of the staging buffer (synchronizes) ...
        void stage( const int32_t* ids_host, const float* values_host, size_t n )
        {
            if ( n > kStage ) throw std::invalid_argument( "RocmTokenBias::stage: more than " + std::to_string( kStage ) + " entries" );
            if ( n )
            {
                rocmCheck( mila_cdna4_memcpy_h2d( stage_ids_->data() + kStage, ids_host, n * 4, context_->getStream() ) );
                rocmCheck( mila_cdna4_memcpy_h2d( stage_values_->data() + kStage, values_host, n * 4, context_->getStream() ) );
                context_->synchronize();
            }
            staged_ = n;
        }
        /// ... and enqueue it: one launch in stream order, no host data
        void commit()
        {
            rocmCheck( mila_cdna4_token_bias_set( data(), 0, 0, static_cast<int>( vocab_ ), stage_ids_->data() + kStage, stage_values_->data() + kStage, static_cast<int>( staged_ ),
                                                  context_->getStream() ) );
        }
        /// the table to the host (synchronizes)
        void read( float* out )
        {
            rocmCheck( mila_cdna4_memcpy_d2h( out, data(), static_cast<size_t>( vocab_ ) * 4, context_->getStream() ) );
            context_->synchronize();
        }
        size_t stateBytes() const { return table_->sizeInBytes() + stage_ids_->sizeInBytes() + stage_values_->sizeInBytes(); }
        static size_t requiredBytes( dim_t vocab ) { return ( static_cast<size_t>( vocab ) + 4 * kStage ) * 4; }
        static constexpr size_t kStage = 1024;
    private:
        ExecutionContext<DeviceType::Rocm>* context_;
        dim_t vocab_;
        size_t staged_{ 0 };
        std::unique_ptr<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>> table_, stage_values_;
        std::unique_ptr<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>> stage_ids_;
    };

    /// The device side of a token automaton for one row (mila_cdna4.h: token automaton): the image (class_of, then next), the state word and the ticket word, and the
    /// effective table `eff` that the biased samplers read in the place of the bias table.  eff, the state and the ticket never move, so a captured step that holds
    /// them sees every later reset; the image is re-allocated only when its size changes, and key() names what a captured step kernel node holds by value (the image
    /// address, S, C).  Everything runs on the context's stream.  upload() and reset() synchronize (they read host memory); compose() and step() are one launch each.
    /// On a draft_tokens network (drafts > 0) eff has one row per chain row and chain_states one word per row: chainCompose() / chainStep() are the two launches
    /// around the tail of a constrained chain step (mila_cdna4.h: the constrained chain step); row 0 and the state word are the one-row step's.
    class RocmTokenAutomaton
    {
    public:
        struct Key { const void* image = nullptr; int S = 0, C = 0; bool operator==( const Key& ) const = default; };
        /// drafts > 0 (a draft_tokens network): eff has drafts + 1 rows of `vocab` floats -- row t the table of chain row t -- and chain_states drafts + 1 words;
        /// drafts == 0 allocates exactly what it always did
        RocmTokenAutomaton( IExecutionContext* ctx, dim_t vocab, dim_t drafts = 0 ) : context_( cast_context<DeviceType::Rocm>( ctx ) ), vocab_( vocab ), drafts_( drafts )
        {
            if ( vocab <= 0 ) throw std::invalid_argument( "RocmTokenAutomaton: need a positive vocabulary" );
            if ( drafts < 0 || drafts > 3 ) throw std::invalid_argument( "RocmTokenAutomaton: 0 .. 3 drafts" );
            (void)narrowToKernelIndex( vocab, "vocab" );
            const auto dev = context_->getDeviceId();
            eff_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ vocab * ( drafts + 1 ) } );
            words_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ 2 } );
            rocmCheck( mila_cdna4_memset_zero( words_->rawData(), 8, context_->getStream() ) );
            for ( dim_t t = 0; t <= drafts; ++t )
                rocmCheck( mila_cdna4_token_bias_fill( eff_->data(), static_cast<size_t>( vocab_ ), static_cast<int>( t ), static_cast<int>( vocab_ ), 0.0f, context_->getStream() ) );
            if ( drafts > 0 )
            {
                chain_states_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ drafts + 1 } );
                rocmCheck( mila_cdna4_memset_zero( chain_states_->rawData(), chain_states_->sizeInBytes(), context_->getStream() ) );
            }
            context_->synchronize();
        }
        /// the image of a validated automaton (TokenAutomaton::validate) onto the device; the state is whatever it was: reset() follows
        void upload( const uint16_t* class_of, const uint16_t* next, int S, int C, int start )
        {
            const size_t bytes = mila_cdna4_token_automaton_bytes( static_cast<int>( vocab_ ), S, C );
            if ( !bytes || !class_of || !next || start < 0 || start >= S ) throw std::invalid_argument( "RocmTokenAutomaton::upload: an automaton outside the limits of mila_cdna4.h" );
            const dim_t words = static_cast<dim_t>( ( bytes + 3 ) / 4 );
            context_->synchronize();      // (no step in flight reads the image that is replaced)
            if ( !image_ || image_->shape()[ 0 ] != words ) image_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( context_->getDeviceId(), shape_t{ words } );
            rocmCheck( mila_cdna4_memcpy_h2d( image_->rawData(), class_of, static_cast<size_t>( vocab_ ) * 2, context_->getStream() ) );
            rocmCheck( mila_cdna4_memcpy_h2d( nextDev(), next, static_cast<size_t>( S ) * static_cast<size_t>( C ) * 2, context_->getStream() ) );
            context_->synchronize();
            S_ = S; C_ = C; start_ = start;
        }
        bool loaded() const noexcept { return image_ != nullptr; }
        Key key() const noexcept { return Key{ image_ ? image_->rawData() : nullptr, S_, C_ }; }
        const float* eff() { return eff_->data(); }
        /// state = start, ticket = 0, eff composed over `base` (nullptr: zeros)
        void reset( const float* base )
        {
            const int32_t w[ 2 ] = { start_, 0 };
            rocmCheck( mila_cdna4_memcpy_h2d( words_->rawData(), w, 8, context_->getStream() ) );
            context_->synchronize();
            compose( base );
        }
        /// eff for the state the word holds: one launch in stream order
        void compose( const float* base )
        {
            requireLoaded();
            rocmCheck( mila_cdna4_token_automaton_compose( eff_->data(), 0, base, 0, classDev(), nextDev(), S_, C_, words_->data(), 1, static_cast<int>( vocab_ ), context_->getStream() ) );
        }
        /// the state advanced by *token_dev and eff composed for it: one launch in stream order (what a captured step holds as a node)
        void step( const float* base, const int32_t* token_dev )
        {
            requireLoaded();
            rocmCheck( mila_cdna4_token_automaton_step( eff_->data(), 0, base, 0, classDev(), nextDev(), S_, C_, words_->data(), token_dev, nullptr,
                                                        reinterpret_cast<uint32_t*>( words_->data() + 1 ), 1, static_cast<int>( vocab_ ), context_->getStream() ) );
        }
        /// the first node of a constrained chain step of T rows fed tok_dev[ 0 .. T - 1 ]: eff rows 1 .. T - 1 and chain_states, one launch
        void chainCompose( const float* base, const int32_t* tok_dev, int T )
        {
            requireChain( T );
            rocmCheck( mila_cdna4_token_automaton_chain_compose( eff_->data(), static_cast<size_t>( vocab_ ), base, 0, classDev(), nextDev(), S_, C_, words_->data(), tok_dev,
                                                                 chain_states_->data(), T, static_cast<int>( vocab_ ), context_->getStream() ) );
        }
        /// behind the accept tail that left result_dev = {count, ...} and tok_dev[ 0 ]: the state word and eff row 0, one launch
        void chainStep( const float* base, const int32_t* tok_dev, const int32_t* result_dev, int T )
        {
            requireChain( T );
            rocmCheck( mila_cdna4_token_automaton_chain_step( eff_->data(), static_cast<size_t>( vocab_ ), base, 0, classDev(), nextDev(), S_, C_, words_->data(), tok_dev,
                                                              chain_states_->data(), result_dev, T, reinterpret_cast<uint32_t*>( words_->data() + 1 ),
                                                              static_cast<int>( vocab_ ), context_->getStream() ) );
        }
        dim_t drafts() const noexcept { return drafts_; }
        /// the state word (synchronizes)
        int32_t readState()
        {
            int32_t s = 0;
            rocmCheck( mila_cdna4_memcpy_d2h( &s, words_->rawData(), 4, context_->getStream() ) );
            context_->synchronize();
            return s;
        }
        /// the effective table to the host (synchronizes)
        void read( float* out )
        {
            rocmCheck( mila_cdna4_memcpy_d2h( out, eff_->data(), static_cast<size_t>( vocab_ ) * 4, context_->getStream() ) );
            context_->synchronize();
        }
        size_t stateBytes() const { return eff_->sizeInBytes() + words_->sizeInBytes() + ( chain_states_ ? chain_states_->sizeInBytes() : 0 ) + ( image_ ? image_->sizeInBytes() : 0 ); }
        /// eff (one row, and one per draft) + the two words (and the chain's state words) + the image rounded up to whole 32-bit words
        size_t requiredBytes() const
        {
            const size_t rows = static_cast<size_t>( drafts_ ) + 1;
            return rows * static_cast<size_t>( vocab_ ) * 4 + 8 + ( drafts_ > 0 ? rows * 4 : 0 ) +
                   ( image_ ? ( ( mila_cdna4_token_automaton_bytes( static_cast<int>( vocab_ ), S_, C_ ) + 3 ) / 4 ) * 4 : 0 );
        }
    private:
        void requireLoaded() const { if ( !image_ ) throw std::logic_error( "RocmTokenAutomaton: no automaton was uploaded" ); }
        void requireChain( int T ) const
        {
            requireLoaded();
            if ( T < 2 || T > drafts_ + 1 ) throw std::invalid_argument( "RocmTokenAutomaton: a chain step takes 2 .. drafts + 1 rows" );
        }
        const uint16_t* classDev() { return reinterpret_cast<const uint16_t*>( image_->rawData() ); }
        uint16_t* nextDev() { return reinterpret_cast<uint16_t*>( image_->rawData() ) + vocab_; }
        ExecutionContext<DeviceType::Rocm>* context_;
        dim_t vocab_, drafts_;
        int S_{ 0 }, C_{ 0 }, start_{ 0 };
        std::unique_ptr<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>> eff_;
        std::unique_ptr<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>> words_, image_, chain_states_;
    };

    /// The rows form of RocmTokenBias (mila_cdna4.h: row requests): one table per row of a rows step and one staging area per row.  `eff` [rows, vocab] is what the
    /// requests samplers read as row b's bias row; `base` [rows, vocab] is what row b's automaton composes eff FROM.  A row WITHOUT an automaton keeps its table in eff
    /// itself (nothing else writes that row); a row WITH one keeps it in base, and RocmTokenAutomatonRows rewrites eff behind every sample.  Both start as zeros (no
    /// bias).  The addresses never move: a captured rows step sees every later update.  apply() synchronizes (it reads host memory); stage() uploads a restore list
    /// ahead of time and commit() enqueues it as one small launch in stream order.
    class RocmTokenBiasRows
    {
    public:
        static constexpr size_t kStage = RocmTokenBias::kStage;
        RocmTokenBiasRows( IExecutionContext* ctx, dim_t vocab, int rows ) : context_( cast_context<DeviceType::Rocm>( ctx ) ), vocab_( vocab ), rows_( rows )
        {
            if ( vocab <= 0 || rows < 1 || rows > 4 ) throw std::invalid_argument( "RocmTokenBiasRows: need a positive vocabulary and 1 .. 4 rows" );
            (void)narrowToKernelIndex( vocab, "vocab" );
            const auto dev = context_->getDeviceId();
            eff_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( rows ), vocab } );
            base_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( rows ), vocab } );
            stage_ids_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( rows ), static_cast<dim_t>( 2 * kStage ) } );
            stage_values_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( rows ), static_cast<dim_t>( 2 * kStage ) } );
            for ( int b = 0; b < rows; ++b ) { fill( eff_->data(), b, 0.0f ); fill( base_->data(), b, 0.0f ); }
            staged_.assign( static_cast<size_t>( rows ), 0 );
            on_.assign( static_cast<size_t>( rows ), 0 );
            to_base_.assign( static_cast<size_t>( rows ), 0 );
            context_->synchronize();
        }
        float* eff() { return eff_->data(); }
        float* base() { return base_->data(); }
        size_t stride() const noexcept { return static_cast<size_t>( vocab_ ); }
        int rows() const noexcept { return rows_; }
        bool on( int b ) const { checkRow( b ); return on_[ static_cast<size_t>( b ) ] != 0; }
        bool any() const noexcept { for ( char c : on_ ) if ( c ) return true; return false; }
        /// row b's whole table: every value `fill`, then values[j] at ids[j]; into base when the row has an automaton (`to_base`), else into eff
        void apply( int b, bool to_base, float fill_value, const int32_t* ids_host, const float* values_host, size_t n )
        {
            checkRow( b );
            float* t = to_base ? base() : eff();
            fill( t, b, fill_value );
            int32_t* ids = stage_ids_->data() + static_cast<size_t>( b ) * 2 * kStage;
            float* values = stage_values_->data() + static_cast<size_t>( b ) * 2 * kStage;
            for ( size_t i0 = 0; i0 < n; i0 += kStage )
            {
                const size_t c = std::min<size_t>( kStage, n - i0 );
                rocmCheck( mila_cdna4_memcpy_h2d( ids, ids_host + i0, c * 4, context_->getStream() ) );
                rocmCheck( mila_cdna4_memcpy_h2d( values, values_host + i0, c * 4, context_->getStream() ) );
                rocmCheck( mila_cdna4_token_bias_set( t, stride(), b, static_cast<int>( vocab_ ), ids, values, static_cast<int>( c ), context_->getStream() ) );
                context_->synchronize();
            }
            on_[ static_cast<size_t>( b ) ] = 1; to_base_[ static_cast<size_t>( b ) ] = to_base ? 1 : 0; staged_[ static_cast<size_t>( b ) ] = 0;
        }
        /// row b without a bias: zeros in both tables
        void clear( int b )
        {
            checkRow( b );
            fill( eff(), b, 0.0f ); fill( base(), b, 0.0f );
            on_[ static_cast<size_t>( b ) ] = 0; to_base_[ static_cast<size_t>( b ) ] = 0; staged_[ static_cast<size_t>( b ) ] = 0;
        }
        /// row b's restore list (at most kStage entries) into the second half of its staging area (synchronizes) ...
        void stage( int b, const int32_t* ids_host, const float* values_host, size_t n )
        {
            checkRow( b );
            if ( n > kStage ) throw std::invalid_argument( "RocmTokenBiasRows::stage: more than " + std::to_string( kStage ) + " entries" );
            if ( n )
            {
                rocmCheck( mila_cdna4_memcpy_h2d( stage_ids_->data() + static_cast<size_t>( b ) * 2 * kStage + kStage, ids_host, n * 4, context_->getStream() ) );
                rocmCheck( mila_cdna4_memcpy_h2d( stage_values_->data() + static_cast<size_t>( b ) * 2 * kStage + kStage, values_host, n * 4, context_->getStream() ) );
                context_->synchronize();
            }
            staged_[ static_cast<size_t>( b ) ] = n;
        }
        /// ... and enqueue it on the table apply() wrote: one launch in stream order, no host data
        void commit( int b )
        {
            checkRow( b );
            rocmCheck( mila_cdna4_token_bias_set( to_base_[ static_cast<size_t>( b ) ] ? base() : eff(), stride(), b, static_cast<int>( vocab_ ),
                                                  stage_ids_->data() + static_cast<size_t>( b ) * 2 * kStage + kStage, stage_values_->data() + static_cast<size_t>( b ) * 2 * kStage + kStage,
                                                  static_cast<int>( staged_[ static_cast<size_t>( b ) ] ), context_->getStream() ) );
        }
        /// row b of eff to the host (synchronizes)
        void read( int b, float* out )
        {
            checkRow( b );
            rocmCheck( mila_cdna4_memcpy_d2h( out, eff() + static_cast<size_t>( b ) * stride(), stride() * 4, context_->getStream() ) );
            context_->synchronize();
        }
        size_t stateBytes() const { return eff_->sizeInBytes() + base_->sizeInBytes() + stage_ids_->sizeInBytes() + stage_values_->sizeInBytes(); }
        static size_t requiredBytes( dim_t vocab, int rows ) { return static_cast<size_t>( rows ) * ( 2 * static_cast<size_t>( vocab ) + 4 * kStage ) * 4; }
    private:
        void checkRow( int b ) const { if ( b < 0 || b >= rows_ ) throw std::invalid_argument( "RocmTokenBiasRows: row " + std::to_string( b ) + " outside 0 .. " + std::to_string( rows_ - 1 ) ); }
        void fill( float* t, int b, float v ) { rocmCheck( mila_cdna4_token_bias_fill( t, stride(), b, static_cast<int>( vocab_ ), v, context_->getStream() ) ); }
        ExecutionContext<DeviceType::Rocm>* context_;
        dim_t vocab_;
        int rows_;
        std::vector<size_t> staged_;
        std::vector<char> on_, to_base_;
        std::unique_ptr<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>> eff_, base_, stage_values_;
        std::unique_ptr<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>> stage_ids_;
    };

    /// The rows form of RocmTokenAutomaton (mila_cdna4.h: row requests): one image, one state word and one ticket word per row, and the descriptor array the rows
    /// step reads.  It owns no table: eff and base are RocmTokenBiasRows'.  set() uploads a validated image, stores the row's descriptor in stream order and puts the
    /// state word to `start`; clear() stores the null descriptor (the row has no automaton: the step does not touch it).  compose() / step() are one launch for all
    /// rows; stepRow() is the one-row entry on row b alone (behind a row's first token).  set() and readState() synchronize.
    class RocmTokenAutomatonRows
    {
    public:
        RocmTokenAutomatonRows( IExecutionContext* ctx, dim_t vocab, int rows ) : context_( cast_context<DeviceType::Rocm>( ctx ) ), vocab_( vocab ), rows_( rows )
        {
            if ( vocab <= 0 || rows < 1 || rows > 4 ) throw std::invalid_argument( "RocmTokenAutomatonRows: need a positive vocabulary and 1 .. 4 rows" );
            (void)narrowToKernelIndex( vocab, "vocab" );
            const auto dev = context_->getDeviceId();
            words_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( 2 * rows ) } );      // states, then tickets
            desc_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( mila_cdna4_token_automaton_rows_bytes( rows ) / 4 ) } );
            rocmCheck( mila_cdna4_memset_zero( words_->rawData(), words_->sizeInBytes(), context_->getStream() ) );
            rocmCheck( mila_cdna4_memset_zero( desc_->rawData(), desc_->sizeInBytes(), context_->getStream() ) );      // null descriptors
            images_.resize( static_cast<size_t>( rows ) );
            shape_.assign( static_cast<size_t>( rows ), Shape{} );
            context_->synchronize();
        }
        bool on( int b ) const { checkRow( b ); return shape_[ static_cast<size_t>( b ) ].S > 0; }
        bool any() const noexcept { for ( auto& s : shape_ ) if ( s.S > 0 ) return true; return false; }
        void set( int b, const uint16_t* class_of, const uint16_t* next, int S, int C, int start )
        {
            checkRow( b );
            const size_t bytes = mila_cdna4_token_automaton_bytes( static_cast<int>( vocab_ ), S, C );
            if ( !bytes || !class_of || !next || start < 0 || start >= S ) throw std::invalid_argument( "RocmTokenAutomatonRows::set: an automaton outside the limits of mila_cdna4.h" );
            const dim_t words = static_cast<dim_t>( ( bytes + 3 ) / 4 );
            context_->synchronize();      // (no step in flight reads the image that is replaced)
            auto& image = images_[ static_cast<size_t>( b ) ];
            if ( !image || image->shape()[ 0 ] != words ) image = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( context_->getDeviceId(), shape_t{ words } );
            uint16_t* cls = reinterpret_cast<uint16_t*>( image->rawData() );
            rocmCheck( mila_cdna4_memcpy_h2d( cls, class_of, static_cast<size_t>( vocab_ ) * 2, context_->getStream() ) );
            rocmCheck( mila_cdna4_memcpy_h2d( cls + vocab_, next, static_cast<size_t>( S ) * static_cast<size_t>( C ) * 2, context_->getStream() ) );
            const int32_t w = start, zero = 0;
            rocmCheck( mila_cdna4_memcpy_h2d( words_->data() + b, &w, 4, context_->getStream() ) );
            rocmCheck( mila_cdna4_memcpy_h2d( words_->data() + rows_ + b, &zero, 4, context_->getStream() ) );
            rocmCheck( mila_cdna4_token_automaton_rows_set( desc_->rawData(), b, cls, cls + vocab_, S, C, static_cast<int>( vocab_ ), context_->getStream() ) );
            context_->synchronize();
            shape_[ static_cast<size_t>( b ) ] = Shape{ S, C };
        }
        void clear( int b )
        {
            checkRow( b );
            rocmCheck( mila_cdna4_token_automaton_rows_set( desc_->rawData(), b, nullptr, nullptr, 0, 0, 0, context_->getStream() ) );
            shape_[ static_cast<size_t>( b ) ] = Shape{};
        }
        /// every row's eff row for the state its word holds (rows without an automaton are not touched): one launch
        void compose( RocmTokenBiasRows& t )
        {
            rocmCheck( mila_cdna4_token_automaton_rows_compose( t.eff(), t.stride(), t.base(), t.stride(), desc_->rawData(), words_->data(), rows_, static_cast<int>( vocab_ ), context_->getStream() ) );
        }
        /// behind the sampler tails of a rows step over rows 0 .. B - 1: the active rows' states advanced by tok_dev[b], their eff rows rewritten; one launch
        void step( RocmTokenBiasRows& t, const int32_t* tok_dev, const int32_t* active_dev, int B )
        {
            rocmCheck( mila_cdna4_token_automaton_rows_step( t.eff(), t.stride(), t.base(), t.stride(), desc_->rawData(), words_->data(), tok_dev, active_dev,
                                                             reinterpret_cast<uint32_t*>( words_->data() + rows_ ), B, static_cast<int>( vocab_ ), context_->getStream() ) );
        }
        /// the one-row step on row b alone, by the token at tok_dev (behind the row's first sample)
        void stepRow( RocmTokenBiasRows& t, int b, const int32_t* tok_dev )
        {
            if ( !on( b ) ) return;
            const uint16_t* cls = reinterpret_cast<const uint16_t*>( images_[ static_cast<size_t>( b ) ]->rawData() );
            const size_t off = static_cast<size_t>( b ) * t.stride();
            rocmCheck( mila_cdna4_token_automaton_step( t.eff() + off, 0, t.base() + off, 0, cls, cls + vocab_, shape_[ static_cast<size_t>( b ) ].S, shape_[ static_cast<size_t>( b ) ].C,
                                                        words_->data() + b, tok_dev, nullptr, reinterpret_cast<uint32_t*>( words_->data() + rows_ + b ), 1, static_cast<int>( vocab_ ),
                                                        context_->getStream() ) );
        }
        /// row b's state word (synchronizes)
        int32_t readState( int b )
        {
            checkRow( b );
            int32_t s = 0;
            rocmCheck( mila_cdna4_memcpy_d2h( &s, words_->data() + b, 4, context_->getStream() ) );
            context_->synchronize();
            return s;
        }
        size_t stateBytes() const
        {
            size_t n = words_->sizeInBytes() + desc_->sizeInBytes();
            for ( auto& i : images_ ) if ( i ) n += i->sizeInBytes();
            return n;
        }
        /// the words and descriptors, plus every uploaded image rounded up to whole 32-bit words
        size_t requiredBytes() const
        {
            size_t n = static_cast<size_t>( rows_ ) * 8 + mila_cdna4_token_automaton_rows_bytes( rows_ );
            for ( size_t b = 0; b < images_.size(); ++b )
                if ( images_[ b ] ) n += static_cast<size_t>( images_[ b ]->shape()[ 0 ] ) * 4;
            return n;
        }
    private:
        struct Shape { int S = 0, C = 0; };
        void checkRow( int b ) const { if ( b < 0 || b >= rows_ ) throw std::invalid_argument( "RocmTokenAutomatonRows: row " + std::to_string( b ) + " outside 0 .. " + std::to_string( rows_ - 1 ) ); }
        ExecutionContext<DeviceType::Rocm>* context_;
        dim_t vocab_;
        int rows_;
        std::vector<Shape> shape_;
        std::unique_ptr<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>> words_, desc_;
        std::vector<std::unique_ptr<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>> images_;
    };

    class RocmSamplingOp : public Operation<DeviceType::Rocm, TensorDataType::FP32>
    {
    public:
        using LogitsTensor = Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>;
        using TokenTensor = Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>;
        RocmSamplingOp( IExecutionContext* ctx, const SamplingOpConfig& cfg ) : Operation( ctx ), cfg_( cfg )
        {
            if ( cfg.vocab_size <= 0 ) throw std::invalid_argument( "RocmSamplingOp: vocabulary size must be positive" );
            scratch_bytes_ = std::max( mila_cdna4_sample_scratch_bytes(), mila_cdna4_sample_stochastic_scratch_bytes( narrowToKernelIndex( cfg.vocab_size, "vocab" ) ) );
            scratch_ = std::make_unique<Tensor<TensorDataType::UINT8, RocmDeviceMemoryResource>>( context_->getDeviceId(), shape_t{ static_cast<dim_t>( scratch_bytes_ ) } );
            seq_dev_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( context_->getDeviceId(), shape_t{ 2 } );      // one 64-bit counter
            rocmCheck( mila_cdna4_memset_zero( seq_dev_->rawData(), 8, context_->getStream() ) );
            void* host = nullptr;
            rocmCheck( mila_cdna4_host_alloc_pinned( &host, sizeof( unsigned long long ) * kSlots ) );
            ring_ = static_cast<unsigned long long*>( host );
            for ( int i = 0; i < kSlots; ++i ) ring_[ i ] = 0;
            context_->synchronize();
        }
        ~RocmSamplingOp() override { if ( ring_ ) mila_cdna4_host_free_pinned( ring_ ); }

        /// logits [.., vocab] -> token_out[0]; r in [0, 1) is drawn by the caller (the reference injects it the same way).  With any filter of `sp` set the call goes to
        /// the filtered entries (mila_cdna4_sample_radix_filtered_fp32 / _sample_argmax_filtered_fp32): penalties read row `row` of `table` and the chosen token is
        /// counted there (penalties without a table: std::invalid_argument); min_p alone needs none and leaves a greedy request as it is.
        void forward( const LogitsTensor& logits, TokenTensor& token_out, const SamplingParams& sp, float r, RocmTokenTable* table = nullptr, int row = 0 ) const
        {
            const int V = narrowToKernelIndex( cfg_.vocab_size, "vocab" );
            if ( static_cast<dim_t>( logits.size() ) < cfg_.vocab_size ) throw std::invalid_argument( "RocmSamplingOp::forward: logits are shorter than the vocabulary" );
            if ( sp.filtered() )
            {
                sp.checkFilters( "RocmSamplingOp::forward" );
                if ( sp.penalized() && !table ) throw std::invalid_argument( "RocmSamplingOp::forward: penalties need a token table" );
                if ( table && static_cast<dim_t>( table->stride() ) != cfg_.vocab_size ) throw std::invalid_argument( "RocmSamplingOp::forward: the token table is of another vocabulary" );
                const mila_sample_filters f = sp.filters();
                uint32_t* words = sp.penalized() ? table->row( row ) : nullptr;
                if ( sp.temperature <= 0.0f || sp.top_k == 1 )
                    rocmCheck( mila_cdna4_sample_argmax_filtered_fp32( logits.data(), token_out.data(), V, cfg_.final_logit_softcap, &f, words, scratch_->rawData(), scratch_bytes_,
                                                                       context_->getStream() ) );
                else
                {
                    // the radix pipeline's workspace: allocated by the first filtered stochastic call, so an op that never sees a filter holds what it always held
                    if ( !radix_scratch_ )
                        radix_scratch_ = std::make_unique<Tensor<TensorDataType::UINT8, RocmDeviceMemoryResource>>( context_->getDeviceId(), shape_t{ static_cast<dim_t>( mila_cdna4_sample_radix_scratch_bytes( V ) ) } );
                    rocmCheck( mila_cdna4_sample_radix_filtered_fp32( logits.data(), token_out.data(), V, cfg_.final_logit_softcap, sp.temperature, sp.top_k, sp.top_p, r, &f, words,
                                                                      radix_scratch_->rawData(), radix_scratch_->sizeInBytes(), context_->getStream() ) );
                }
                return;
            }
            if ( sp.temperature <= 0.0f || sp.top_k == 1 )
                rocmCheck( mila_cdna4_sample_argmax_fp32( logits.data(), token_out.data(), V, scratch_->rawData(), scratch_bytes_, context_->getStream() ) );
            else
                rocmCheck( mila_cdna4_sample_stochastic_fp32( logits.data(), token_out.data(), V, cfg_.final_logit_softcap, sp.temperature, sp.top_k, sp.top_p, r, scratch_->rawData(),
                                                              scratch_bytes_, context_->getStream() ) );
        }
        void enqueueForward( const LogitsTensor& logits, TokenTensor& token_out, const SamplingParams& sp, float r, RocmTokenTable* table = nullptr, int row = 0 )
        {
            forward( logits, token_out, sp, r, table, row );
            rocmCheck( mila_cdna4_snapshot_token( token_out.data(), reinterpret_cast<unsigned long long*>( seq_dev_->rawData() ), ring_, kSlots, context_->getStream() ) );
            ++enqueued_;
        }
        int32_t awaitToken()
        {
            if ( awaited_ >= enqueued_ ) throw std::logic_error( "RocmSamplingOp::awaitToken: no outstanding enqueueForward()" );
            const uint64_t seq = ++awaited_;
            volatile unsigned long long* slot = ring_ + ( seq % kSlots );
            const auto t0 = std::chrono::steady_clock::now();
            for ( uint64_t spins = 0;; ++spins )
            {
                const unsigned long long v = __atomic_load_n( slot, __ATOMIC_ACQUIRE );
                if ( ( v >> 32 ) == ( seq & 0xffffffffull ) ) return static_cast<int32_t>( static_cast<uint32_t>( v ) );
                if ( ( spins & 1023 ) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds( 20 ) )
                    throw std::runtime_error( "RocmSamplingOp::awaitToken: the device did not publish a token within 20 s" );
            }
        }
    private:
        static constexpr int kSlots = 4;
        SamplingOpConfig cfg_;
        size_t scratch_bytes_{ 0 };
        std::unique_ptr<Tensor<TensorDataType::UINT8, RocmDeviceMemoryResource>> scratch_;
        mutable std::unique_ptr<Tensor<TensorDataType::UINT8, RocmDeviceMemoryResource>> radix_scratch_;      // filtered stochastic calls only
        std::unique_ptr<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>> seq_dev_;
        unsigned long long* ring_{ nullptr };
        uint64_t enqueued_{ 0 }, awaited_{ 0 };
    };
    template<> struct OperationTraits<OperationType::SamplingOp, DeviceType::Rocm, TensorDataType::FP32> { using type = RocmSamplingOp; };

    // ---------------------------------------------------------------------------------------
    // Token log-probabilities (mila_cdna4_token_logprobs_*, csrc/logprobs.hip): the log-probability of the token a step chose and of the top-n alternatives, from the
    // fp32 logits on the device.  The op owns the kernels' scratch (max_rows regions at the widest list) and the device outputs of the rows form; the publish form
    // writes a record into a caller-owned host-visible ring instead.  Both are two launches on the context's stream; nothing synchronizes.
    // ---------------------------------------------------------------------------------------
    struct TokenLogprobsOpConfig { dim_t vocab_size{ 0 }; float final_logit_softcap{ 0.0f }; int max_rows{ 1 }; };

    class RocmTokenLogprobsOp : public Operation<DeviceType::Rocm, TensorDataType::FP32>
    {
    public:
        static constexpr int kMaxTop = 20;
        RocmTokenLogprobsOp( IExecutionContext* ctx, const TokenLogprobsOpConfig& cfg ) : Operation( ctx ), cfg_( cfg )
        {
            if ( cfg.vocab_size <= 0 ) throw std::invalid_argument( "RocmTokenLogprobsOp: vocabulary size must be positive" );
            if ( cfg.max_rows < 1 || cfg.max_rows > 4 ) throw std::invalid_argument( "RocmTokenLogprobsOp: 1 .. 4 rows" );
            const int V = narrowToKernelIndex( cfg.vocab_size, "vocab" );
            scratch_bytes_ = mila_cdna4_token_logprobs_scratch_bytes( cfg.max_rows, V, maxTop() );
            const auto dev = context_->getDeviceId();
            scratch_ = std::make_unique<Tensor<TensorDataType::UINT8, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( scratch_bytes_ ) } );
            logprob_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ cfg.max_rows } );
            top_ids_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ cfg.max_rows, kMaxTop } );
            top_logprobs_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ cfg.max_rows, kMaxTop } );
        }
        /// the longest list this vocabulary allows
        int maxTop() const { return static_cast<int>( std::min<dim_t>( kMaxTop, cfg_.vocab_size ) ); }
        void checkTop( int top_n ) const
        {
            if ( top_n < 0 || top_n > maxTop() ) throw std::invalid_argument( "token log-probabilities: top_n " + std::to_string( top_n ) + " outside 0 .. " + std::to_string( maxTop() ) );
        }
        /// rows 0 .. rows - 1 of `logits` (logits_stride floats apart) report tokens_dev[ b ] into the op's outputs: logprob [ b ], ids / logprobs [ b * top_n .. ).  A row
        /// whose active word is 0, or whose index is >= *count_dev, keeps what it held (either pointer may be null)
        void forward( const float* logits, size_t logits_stride, const int32_t* tokens_dev, int rows, int top_n, const int32_t* active_dev, const int32_t* count_dev )
        {
            checkTop( top_n );
            if ( rows < 1 || rows > cfg_.max_rows ) throw std::invalid_argument( "RocmTokenLogprobsOp::forward: rows outside 1 .. max_rows" );
            rocmCheck( mila_cdna4_token_logprobs_rows_fp32( logits, logits_stride, tokens_dev, rows, narrowToKernelIndex( cfg_.vocab_size, "vocab" ), cfg_.final_logit_softcap, top_n,
                                                            active_dev, count_dev, logprob_->data(), top_ids_->data(), top_logprobs_->data(), scratch_->rawData(), scratch_bytes_,
                                                            context_->getStream() ) );
        }
        /// the one-row form of a decode-ahead loop: one record of recordWords() 32-bit words into slot *seq_dev % ring_size of the host-visible ring, the tag last
        void publish( const float* logits, const int32_t* token_dev, int top_n, const unsigned long long* seq_dev, uint32_t* ring, int ring_size )
        {
            checkTop( top_n );
            rocmCheck( mila_cdna4_token_logprobs_publish_fp32( logits, token_dev, narrowToKernelIndex( cfg_.vocab_size, "vocab" ), cfg_.final_logit_softcap, top_n, seq_dev, ring,
                                                               ring_size, scratch_->rawData(), scratch_bytes_, context_->getStream() ) );
        }
        static int recordWords() { return mila_cdna4_token_logprobs_record_words(); }
        /// the outputs of the last forward( .., rows, top_n, .. ) to the host (synchronizes): logprob [rows], ids / logprobs [rows * top_n]; null pointers are skipped
        void read( int rows, int top_n, float* logprob, int32_t* top_ids, float* top_logprobs ) const
        {
            const size_t list = static_cast<size_t>( rows ) * static_cast<size_t>( top_n );
            if ( logprob ) rocmCheck( mila_cdna4_memcpy_d2h( logprob, logprob_->data(), static_cast<size_t>( rows ) * 4, context_->getStream() ) );
            if ( top_ids && list ) rocmCheck( mila_cdna4_memcpy_d2h( top_ids, top_ids_->data(), list * 4, context_->getStream() ) );
            if ( top_logprobs && list ) rocmCheck( mila_cdna4_memcpy_d2h( top_logprobs, top_logprobs_->data(), list * 4, context_->getStream() ) );
            context_->synchronize();
        }
        /// device bytes the op holds
        size_t stateBytes() const { return scratch_->sizeInBytes() + logprob_->sizeInBytes() + top_ids_->sizeInBytes() + top_logprobs_->sizeInBytes(); }
    private:
        TokenLogprobsOpConfig cfg_;
        size_t scratch_bytes_{ 0 };
        std::unique_ptr<Tensor<TensorDataType::UINT8, RocmDeviceMemoryResource>> scratch_;
        std::unique_ptr<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>> logprob_, top_logprobs_;
        std::unique_ptr<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>> top_ids_;
    };

    // ---------------------------------------------------------------------------------------
    // Prompt log-probabilities (mila_cdna4_lm_head_score_bf16, csrc/lm_head_score.hip): the lm_head over the rows of a prefill chunk as a GEMM that keeps the softmax
    // statistics and stores no logit.  The op owns the kernel's scratch and its device outputs; they are allocated on FIRST use (a model that never scores holds
    // none of them) and counted in stateBytes() from then on.  Two launches on the context's stream; nothing synchronizes.
    // ---------------------------------------------------------------------------------------
    struct LmHeadScoreOpConfig { dim_t vocab_size{ 0 }; dim_t input_features{ 0 }; float final_logit_softcap{ 0.0f }; dim_t max_rows{ 1 }; };

    class RocmLmHeadScoreOp : public Operation<DeviceType::Rocm, TensorDataType::FP32>
    {
    public:
        RocmLmHeadScoreOp( IExecutionContext* ctx, const LmHeadScoreOpConfig& cfg ) : Operation( ctx ), cfg_( cfg )
        {
            if ( cfg.vocab_size <= 0 || cfg.input_features <= 0 ) throw std::invalid_argument( "RocmLmHeadScoreOp: vocabulary size and input features must be positive" );
            if ( cfg.max_rows < 1 ) throw std::invalid_argument( "RocmLmHeadScoreOp: max_rows must be positive" );
        }
        /// rows 0 .. rows - 1 of x (bf16, x_stride elements apart, already normed) against the table W [vocab, K] in `fmt` (0 bf16, 1 e4m3 + scales): the log-probability
        /// of targets_dev[ r ] (-1 = none: NaN) and, with argmax, the greedy token and its log-probability, into the op's outputs
        void forward( const uint16_t* x, size_t x_stride, const void* W, const float* scales, int fmt, const int32_t* targets_dev, dim_t rows, bool argmax )
        {
            if ( rows < 1 || rows > cfg_.max_rows ) throw std::invalid_argument( "RocmLmHeadScoreOp::forward: rows outside 1 .. max_rows" );
            ensure();
            rocmCheck( mila_cdna4_lm_head_score_bf16( x, x_stride, W, scales, fmt, narrowToKernelIndex( cfg_.input_features, "K" ), narrowToKernelIndex( cfg_.vocab_size, "vocab" ),
                                                      targets_dev, narrowToKernelIndex( rows, "rows" ), cfg_.final_logit_softcap, logprob_->data(),
                                                      argmax ? argmax_->data() : nullptr, argmax ? argmax_logprob_->data() : nullptr, scratch_->rawData(), scratch_bytes_,
                                                      context_->getStream() ) );
        }
        /// the outputs of the last forward( .., rows, .. ) to the host (synchronizes); null pointers are skipped
        void read( dim_t rows, float* logprob, int32_t* argmax, float* argmax_logprob ) const
        {
            const size_t n = static_cast<size_t>( rows ) * 4;
            if ( logprob ) rocmCheck( mila_cdna4_memcpy_d2h( logprob, logprob_->data(), n, context_->getStream() ) );
            if ( argmax ) rocmCheck( mila_cdna4_memcpy_d2h( argmax, argmax_->data(), n, context_->getStream() ) );
            if ( argmax_logprob ) rocmCheck( mila_cdna4_memcpy_d2h( argmax_logprob, argmax_logprob_->data(), n, context_->getStream() ) );
            context_->synchronize();
        }
        /// device bytes the op holds: 0 until the first forward
        size_t stateBytes() const { return scratch_ ? scratch_->sizeInBytes() + logprob_->sizeInBytes() + argmax_->sizeInBytes() + argmax_logprob_->sizeInBytes() : 0; }
        size_t scratchBytes() const { return scratch_bytes_; }
    private:
        void ensure()
        {
            if ( scratch_ ) return;
            scratch_bytes_ = mila_cdna4_lm_head_score_scratch_bytes( narrowToKernelIndex( cfg_.max_rows, "rows" ), narrowToKernelIndex( cfg_.vocab_size, "vocab" ) );
            const auto dev = context_->getDeviceId();
            auto scratch = std::make_unique<Tensor<TensorDataType::UINT8, RocmDeviceMemoryResource>>( dev, shape_t{ static_cast<dim_t>( scratch_bytes_ ) } );
            logprob_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ cfg_.max_rows } );
            argmax_ = std::make_unique<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>>( dev, shape_t{ cfg_.max_rows } );
            argmax_logprob_ = std::make_unique<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>>( dev, shape_t{ cfg_.max_rows } );
            scratch_ = std::move( scratch );
        }
        LmHeadScoreOpConfig cfg_;
        size_t scratch_bytes_{ 0 };
        std::unique_ptr<Tensor<TensorDataType::UINT8, RocmDeviceMemoryResource>> scratch_;
        std::unique_ptr<Tensor<TensorDataType::FP32, RocmDeviceMemoryResource>> logprob_, argmax_logprob_;
        std::unique_ptr<Tensor<TensorDataType::INT32, RocmDeviceMemoryResource>> argmax_;
    };

    /// GPT-2 attention on packed QKV (new BF16 row; the reference's CUDA MHA is FP32-only, OPS/OperationTraits.Cuda.ixx:274-282) with the KV-cache
    /// interface of CudaMultiHeadAttentionOp (OPS/Attention/MHA/CudaMhaOp.ixx:107-380: IPositionalUnaryOp::prefill / decode + IKvCacheLifecycle)
    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    class RocmMultiHeadAttentionOp : public Operation<DeviceType::Rocm, TPrecision>
    {
        using Operation<DeviceType::Rocm, TPrecision>::context_;
        static constexpr bool kFp32 = TPrecision == TensorDataType::FP32;      // the reference's own (and only) CUDA MHA row is FP32 (OperationTraits.Cuda.ixx:274-282)
    public:
        using TensorType = RocmTensor<TPrecision>;
        RocmMultiHeadAttentionOp( IExecutionContext* ctx, dim_t model_dim, dim_t num_heads ) : Operation<DeviceType::Rocm, TPrecision>( ctx ), C_( model_dim ), NH_( num_heads )
        {
            if ( model_dim <= 0 || num_heads <= 0 || model_dim % num_heads != 0 ) throw std::invalid_argument( "RocmMultiHeadAttentionOp: model_dim must be a positive multiple of num_heads" );
        }
        /// the built [B, T, 3C] shape bounds every later call (CudaMhaOp.ixx:423-447)
        void build( const BuildContext& ctx )
        {
            const auto& s = ctx.inputShape();
            if ( s.size() != 3 || s[ 2 ] != 3 * C_ ) throw std::invalid_argument( "RocmMultiHeadAttentionOp::build: expected [B, T, 3C]" );
            B_ = s[ 0 ]; T_ = s[ 1 ];
            cached_seq_len_ = 0; kv_cache_enabled_ = false;
        }
        void forward( const TensorType& qkv, TensorType& out ) const
        {
            const auto& s = qkv.shape();
            if ( s.size() != 3 || s[ 2 ] != 3 * C_ ) throw std::invalid_argument( "RocmMultiHeadAttentionOp::forward: expected [B, T, 3C]" );
            if constexpr ( kFp32 ) rocmCheck( mila_cdna4_mha_fp32( static_cast<float*>( out.rawData() ), static_cast<const float*>( qkv.rawData() ), (int)s[ 0 ], (int)s[ 1 ], (int)C_, (int)NH_, context_->getStream() ) );
            else rocmCheck( mila_cdna4_mha_bf16( static_cast<uint16_t*>( out.rawData() ), static_cast<const uint16_t*>( qkv.rawData() ), (int)s[ 0 ], (int)s[ 1 ], (int)C_, (int)NH_, context_->getStream() ) );
        }

        // ---- IKvCacheLifecycle (CudaMhaOp.ixx:112-143) ----
        void initializeKvCache( dim_t batch_size, dim_t max_sequence_length )
        {
            if ( batch_size != B_ ) throw std::invalid_argument( "RocmMultiHeadAttentionOp::initializeKvCache batch size must match the built shape" );
            if ( max_sequence_length <= 0 || max_sequence_length > T_ ) throw std::invalid_argument( "RocmMultiHeadAttentionOp::initializeKvCache max_sequence_length out of range" );
            if ( !k_cache_ || active_max_seq_len_ != max_sequence_length )
            {
                const shape_t cs{ B_, NH_, max_sequence_length, C_ / NH_ };
                k_cache_ = std::make_unique<TensorType>( context_->getDeviceId(), cs );
                v_cache_ = std::make_unique<TensorType>( context_->getDeviceId(), cs );
            }
            active_max_seq_len_ = max_sequence_length;
            cached_seq_len_ = 0;
            kv_cache_enabled_ = true;
        }
        void resetKvCache() noexcept { cached_seq_len_ = 0; }
        bool rewindKvCache( dim_t position ) noexcept
        {
            if ( position < 0 || position > cached_seq_len_ ) return false;
            cached_seq_len_ = position;
            return true;
        }
        dim_t cacheLength() const noexcept { return cached_seq_len_; }
        size_t stateBytes() const noexcept { return ( k_cache_ ? k_cache_->sizeInBytes() : 0 ) + ( v_cache_ ? v_cache_->sizeInBytes() : 0 ); }

        // ---- IPositionalUnaryOp ----
        /// the whole prompt [B, T' <= max_seq, 3C]: causal attention + the prompt's K / V rows into the cache (CudaMhaOp.ixx:145-232)
        void prefill( const TensorType& qkv, TensorType& out )
        {
            ensureKvCacheEnabled();
            const auto& s = qkv.shape();
            if ( s.size() != 3 || s[ 0 ] != B_ || s[ 2 ] != 3 * C_ || s[ 1 ] <= 0 || s[ 1 ] > active_max_seq_len_ )
                throw std::invalid_argument( "RocmMultiHeadAttentionOp::prefill: input must be [B, T <= max_sequence_length, 3C]" );
            mila_stream_t st = context_->getStream();
            if constexpr ( kFp32 )
            {
                const auto* x = static_cast<const float*>( qkv.rawData() );
                rocmCheck( mila_cdna4_mha_fp32( static_cast<float*>( out.rawData() ), x, (int)B_, (int)s[ 1 ], (int)C_, (int)NH_, st ) );
                rocmCheck( mila_cdna4_mha_kv_write_fp32( static_cast<float*>( k_cache_->rawData() ), static_cast<float*>( v_cache_->rawData() ), x, (int)B_, (int)s[ 1 ], (int)C_, (int)NH_, 0,
                                                         (int)active_max_seq_len_, st ) );
            }
            else
            {
                const auto* x = static_cast<const uint16_t*>( qkv.rawData() );
                rocmCheck( mila_cdna4_mha_bf16( static_cast<uint16_t*>( out.rawData() ), x, (int)B_, (int)s[ 1 ], (int)C_, (int)NH_, st ) );
                rocmCheck( mila_cdna4_mha_kv_write_bf16( static_cast<uint16_t*>( k_cache_->rawData() ), static_cast<uint16_t*>( v_cache_->rawData() ), x, (int)B_, (int)s[ 1 ], (int)C_, (int)NH_, 0,
                                                         (int)active_max_seq_len_, st ) );
            }
            cached_seq_len_ = s[ 1 ];
        }
        /// one token per sequence [B, 1, 3C] at absolute `position`: appends its K / V, attends to keys 0 .. position (CudaMhaOp.ixx:252-380)
        void decode( const TensorType& qkv, TensorType& out, dim_t position )
        {
            ensureKvCacheEnabled();
            const auto& s = qkv.shape();
            if ( s.size() != 3 || s[ 0 ] != B_ || s[ 1 ] != 1 || s[ 2 ] != 3 * C_ ) throw std::invalid_argument( "RocmMultiHeadAttentionOp::decode: input must be [B, 1, 3C]" );
            if ( position < 0 || position >= active_max_seq_len_ ) throw std::invalid_argument( "RocmMultiHeadAttentionOp::decode position out of range" );
            if constexpr ( kFp32 )
                rocmCheck( mila_cdna4_mha_decode_fp32( static_cast<float*>( out.rawData() ), static_cast<const float*>( qkv.rawData() ), static_cast<float*>( k_cache_->rawData() ),
                                                       static_cast<float*>( v_cache_->rawData() ), (int)B_, (int)C_, (int)NH_, (int)active_max_seq_len_, (int)position, context_->getStream() ) );
            else
            {
                const size_t need = mila_cdna4_mha_decode_scratch_bytes( (int)B_, (int)C_, (int)NH_ );
                void* scratch = context_->getScratch( need );      // fetched per call, never cached
                rocmCheck( mila_cdna4_mha_decode_bf16( static_cast<uint16_t*>( out.rawData() ), static_cast<const uint16_t*>( qkv.rawData() ), static_cast<uint16_t*>( k_cache_->rawData() ),
                                                       static_cast<uint16_t*>( v_cache_->rawData() ), scratch, need, (int)B_, (int)C_, (int)NH_, (int)active_max_seq_len_, (int)position,
                                                       context_->getStream() ) );
            }
            if ( position + 1 > cached_seq_len_ ) cached_seq_len_ = position + 1;
        }
    private:
        void ensureKvCacheEnabled() const { if ( !kv_cache_enabled_ ) throw std::runtime_error( "RocmMultiHeadAttentionOp: initializeKvCache() must be called first" ); }
        dim_t C_, NH_;
        dim_t B_{ 0 }, T_{ 0 }, active_max_seq_len_{ 0 }, cached_seq_len_{ 0 };
        bool kv_cache_enabled_{ false };
        std::unique_ptr<TensorType> k_cache_, v_cache_;
    };
    template<TensorDataType TPrecision> requires RocmPrecision<TPrecision>
    struct OperationTraits<OperationType::MultiHeadAttentionOp, DeviceType::Rocm, TPrecision> { using type = RocmMultiHeadAttentionOp<TPrecision>; };
}
