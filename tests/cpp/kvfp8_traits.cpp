// Compile-time facts of the FP8 KV cache policy in the host mirror (compiled, not run, by tests/test_kvfp8_cpu.py with the host flags of mila_amd/build.py):
// the GroupedQueryAttentionOp trait for the three KV policies, the QuantKvPolicy concept, and the model's block aliases.  With -DKVFP8_ASK_E5M2 the translation
// unit asks for the one storage type the row rejects, and must fail with the row's message.
#include <type_traits>

#include "Mila/Gemma.h"

using namespace Mila::Dnn;
using Compute::OperationTraits;
using Compute::OperationType;
namespace Kv = Quant::KvCache;

template<typename P> using GqaOpOf = typename OperationTraits<OperationType::GroupedQueryAttentionOp, DeviceType::Rocm, TensorDataType::BF16, P>::type;
template<typename P> using GqaOf = GroupedQueryAttention<DeviceType::Rocm, TensorDataType::BF16, P>;

// the trait: the ring policies keep their op, the FP8 policy has its own
static_assert( std::is_same_v<GqaOpOf<Kv::NoKvCompression>, Compute::RocmGqaOp<false>> );
static_assert( std::is_same_v<GqaOpOf<Kv::SlidingWindowKvCache>, Compute::RocmGqaOp<true>> );
static_assert( std::is_same_v<GqaOpOf<Kv::PerChannelKvFp8<>>, Compute::RocmGqaKvFp8Op> );
static_assert( std::is_same_v<GqaOpOf<Kv::PerChannelKvFp8<TensorDataType::FP8_E4M3>>, Compute::RocmGqaKvFp8Op> );
static_assert( std::is_same_v<GqaOf<Kv::PerChannelKvFp8<>>::OpType, Compute::RocmGqaKvFp8Op> );
static_assert( std::is_same_v<GqaOf<Kv::NoKvCompression>::OpType, Compute::RocmGqaOp<false>> );
static_assert( !std::is_base_of_v<Compute::RocmGqaOpBase, Compute::RocmGqaKvFp8Op> );      // a sibling: it owns no bf16 cache

// the policy type
static_assert( Kv::QuantKvPolicy<Kv::PerChannelKvFp8<>> );
static_assert( !Kv::QuantKvPolicy<Kv::NoKvCompression> && !Kv::QuantKvPolicy<Kv::SlidingWindowKvCache> );
static_assert( Kv::PerChannelKvFp8<>::kIsActive && Kv::PerChannelKvFp8<>::kPerHeadPerToken && Kv::PerChannelKvFp8<>::kSymmetric && !Kv::PerChannelKvFp8<>::kBoundedRing );
static_assert( Kv::PerChannelKvFp8<>::kStorageDtype == TensorDataType::FP8_E4M3 && Kv::PerChannelKvFp8<>::kScaleDtype == TensorDataType::FP32 );
static_assert( Kv::PerChannelKvFp8<TensorDataType::FP8_E5M2>::kStorageDtype == TensorDataType::FP8_E5M2 );      // naming the policy is fine; asking for its op row is not

// the op's surface: what RocmGqaOpBase offers
template<typename Op>
concept GqaOpSurface = requires( Op& op, const typename Op::TensorType& t, typename Op::TensorType& o )
{
    op.initializeKvCache( 1, dim_t{ 8 }, dim_t{ 8 } );
    op.resetKvCache();
    op.rewindKvCache( dim_t{ 0 } );
    { op.cacheLength() } -> std::same_as<dim_t>;
    { op.cacheCapacity() } -> std::same_as<dim_t>;
    op.prefill( t, t, t, o, 1, 0 );
    op.decode( t, t, t, o, 0 );
    op.attendDecode( t, o, 0 );
    op.prefillFromCache( t, o, 1, 0 );
    { op.keyCache() } -> std::same_as<uint16_t*>;
    { op.valueCache() } -> std::same_as<uint16_t*>;
    { op.stateBytes() } -> std::same_as<size_t>;
    { op.requiredStateBytes( 1, dim_t{ 8 }, dim_t{ 8 } ) } -> std::same_as<size_t>;
};
static_assert( GqaOpSurface<Compute::RocmGqaOp<false>> && GqaOpSurface<Compute::RocmGqaKvFp8Op> );

// the Gemma model is not wired to the policy here: its block aliases are what they were
using Net = GemmaTransformer<Quant::Weight::NoWeightQuant>;
static_assert( std::is_same_v<Net::LocalBlockType, GemmaBlock<DeviceType::Rocm, TensorDataType::BF16, false, Quant::Weight::NoWeightQuant, Kv::NoKvCompression>> );
static_assert( std::is_same_v<Net::BoundedLocalBlockType, GemmaBlock<DeviceType::Rocm, TensorDataType::BF16, false, Quant::Weight::NoWeightQuant, Kv::SlidingWindowKvCache>> );
static_assert( std::is_same_v<Net::GlobalBlockType, GemmaBlock<DeviceType::Rocm, TensorDataType::BF16, true, Quant::Weight::NoWeightQuant, Kv::NoKvCompression>> );
static_assert( std::is_same_v<Net::LocalBlockType::AttentionType::OpType, Compute::RocmGqaOp<false>> && std::is_same_v<Net::BoundedLocalBlockType::AttentionType::OpType, Compute::RocmGqaOp<true>> &&
               std::is_same_v<Net::GlobalBlockType::AttentionType::OpType, Compute::RocmGqaOp<false>> );

#ifdef KVFP8_ASK_E5M2
using Rejected = GqaOpOf<Kv::PerChannelKvFp8<TensorDataType::FP8_E5M2>>;
#endif

int main() { return 0; }
