// Compile-time facts of the FP8 KV cache in the Gemma model (compiled, not run, by tests/test_gemma_kvfp8_cpu.py with the host flags of mila_amd/build.py): the two
// block aliases on PerChannelKvFp8<> instantiate and resolve to the FP8 KV cache op, the blocks offer the fp8 cache surface behind GemmaBlockBase, and the switch
// exists in GemmaConfig and GemmaModelConfig.
#include <type_traits>

#include "Mila/GemmaModel.h"

using namespace Mila::Dnn;
namespace Kv = Quant::KvCache;

template<typename W> struct Facts
{
    using Net = GemmaTransformer<W>;
    using Local = typename Net::KvFp8LocalBlockType;
    using Global = typename Net::KvFp8GlobalBlockType;
    static_assert( std::is_same_v<Local, GemmaBlock<DeviceType::Rocm, TensorDataType::BF16, false, W, Kv::PerChannelKvFp8<>>> );
    static_assert( std::is_same_v<Global, GemmaBlock<DeviceType::Rocm, TensorDataType::BF16, true, W, Kv::PerChannelKvFp8<>>> );
    static_assert( std::is_same_v<typename Local::AttentionType::OpType, Compute::RocmGqaKvFp8Op> && std::is_same_v<typename Global::AttentionType::OpType, Compute::RocmGqaKvFp8Op> );
    static_assert( Local::kKvFp8 && Global::kKvFp8 && !Net::LocalBlockType::kKvFp8 && !Net::BoundedLocalBlockType::kKvFp8 && !Net::GlobalBlockType::kKvFp8 );
    static_assert( std::is_base_of_v<typename Net::Layer, Local> && std::is_base_of_v<typename Net::Layer, Global> );
    // the aliases instantiate: every member of both blocks, the virtual fp8 surface included
    static constexpr size_t kSizes = sizeof( Local ) + sizeof( Global );
};
template struct Facts<Quant::Weight::NoWeightQuant>;
template struct Facts<Quant::Weight::PerChannelFp8<>>;
template struct Facts<Quant::Weight::PerGroupFp4<128>>;
namespace Mila::Dnn
{
    template class GemmaBlock<DeviceType::Rocm, TensorDataType::BF16, false, Quant::Weight::NoWeightQuant, Quant::KvCache::PerChannelKvFp8<>>;
    template class GemmaBlock<DeviceType::Rocm, TensorDataType::BF16, true, Quant::Weight::NoWeightQuant, Quant::KvCache::PerChannelKvFp8<>>;
}

// the block's fp8 surface, whatever its policy
template<typename L>
concept KvFp8Surface = requires( L& l, const typename L::TensorType& q, typename L::TensorType& o )
{
    { l.kvFp8() } -> std::same_as<bool>;
    { l.keyCacheFp8() } -> std::same_as<uint8_t*>;
    { l.valueCacheFp8() } -> std::same_as<uint8_t*>;
    { l.keyScales() } -> std::same_as<float*>;
    { l.valueScales() } -> std::same_as<float*>;
    l.prefillFromCache( q, o, 1, 0 );
};
static_assert( KvFp8Surface<GemmaTransformer<Quant::Weight::NoWeightQuant>::Layer> );

// the op: accessors for the four arrays, the attention-only prefill and device-position decode
template<typename Op>
concept KvFp8OpSurface = requires( Op& op, const typename Op::TensorType& q, typename Op::TensorType& o, const int32_t* pos )
{
    { op.keyBytes() } -> std::same_as<uint8_t*>;
    { op.valueBytes() } -> std::same_as<uint8_t*>;
    { op.keyScaleData() } -> std::same_as<float*>;
    { op.valueScaleData() } -> std::same_as<float*>;
    op.attendPrefill( q, o, 1, 0 );
    op.attendDecode( q, o, 0 );
    op.attendDecodeAt( q, o, pos, 1 );
};
static_assert( KvFp8OpSurface<Compute::RocmGqaKvFp8Op> );

// the switch
static_assert( std::is_same_v<decltype( GemmaConfig{}.kv_fp8 ), bool> );
static_assert( std::is_same_v<decltype( std::declval<GemmaModelConfig&>().withKvFp8( true ) ), GemmaModelConfig&> );
static_assert( std::is_same_v<decltype( std::declval<const GemmaModelConfig&>().kvFp8() ), bool> );

int main()
{
    GemmaConfig c;
    return c.kv_fp8 || GemmaModelConfig( 64 ).kvFp8() ? 1 : 0;      // off by default
}
