// L6 caller of the hot path: GemmaModel -- load a pretrained artifact at a deployment configuration, then generate.  Mirrors
//   Models/GemmaModel.ixx:137-170 (fromPretrained -> dispatchWeightQuantization), :604-665 (fromPretrainedImpl: artifact / policy check, geometry from
//   the checkpoint metadata, context-length check, build, loadParameters), :439-568 (onGenerating: prompt check, stop set, transparent KV prefix reuse,
//   the decode-ahead pipeline, the four GenerateStatus outcomes), :750-770 (EOS / end-of-turn stop set, final logit softcap at the sampler);
//   Models/QuantizationDispatch.ixx:34-95; Core/LanguageModelConfig.ixx:88-230; Core/GenerateStatus.ixx; Components/Transformers/{GenerateParams,SamplingParams}.ixx.
// MI355X form of the decode-ahead pipeline: a greedy request runs the captured hipGraph whose last node is the device sampler (the next
// token never leaves the device) and publishes it into a host-visible ring (sequence number << 32 | token, one system-scope store); the host
// polls its slot while the next step is already running: no event, no copy, no stream wait on the decode path.  A stochastic request runs the same loop: its captured
// step ends with the radix sampler (mila_cdna4_sample_radix_advance_fp32), whose uniform draw the host writes into a second host-visible ring before each replay.
// The rows step of generateBatch and the chain step of speculative sampling end in the same sampler run over their rows (mila_cdna4_sample_radix_rows_advance_fp32,
// mila_cdna4_sample_radix_chain_accept_fp32), one host-written draw per row.
#pragma once

#include <atomic>
#include <bit>
#include <chrono>
#include <cstring>
#include <thread>
#include <optional>
#include <random>
#include <span>
#include <unordered_map>
#include <unordered_set>
#include <memory>
#include <variant>

#include "Gemma.h"
#include "PrefixCache.h"
#include "RequestQueue.h"
#include "TokenAutomaton.h"
#include "TokenBias.h"

namespace Mila::Dnn
{
    enum class WeightQuantization { None, FP8, FP4 };
    enum class KvCacheCompression { None, FP8 };
    inline const char* weightQuantizationName( WeightQuantization wq )
    {
        switch ( wq ) { case WeightQuantization::FP8: return "per_channel_fp8_e4m3"; case WeightQuantization::FP4: return "per_group_fp4_128"; default: return "none"; }
    }

    enum class [[nodiscard]] GenerateStatus : int32_t { Success = 0, MaxNewTokensReached, ContextOverflow, ClientCancelled };
    inline std::string_view to_string( GenerateStatus s )
    {
        switch ( s )
        {
            case GenerateStatus::Success: return "stop";
            case GenerateStatus::MaxNewTokensReached: return "length";
            case GenerateStatus::ContextOverflow: return "context_limit";
            case GenerateStatus::ClientCancelled: return "cancelled";
        }
        return "unknown";
    }

    struct SamplingParams
    {
        float temperature = 1.0f;
        int top_k = 0;        ///< 0 disables top-k truncation; 1 == greedy
        float top_p = 1.0f;   ///< 1.0 disables nucleus truncation
        // The sampling filters (Specifications/TokenSampling.md 3.3; include/mila_cdna4.h: sampling filters), neutral by default.  The penalties read a per-request
        // token table on the device (bit 31: the token occurs in the prompt, bits 0 .. 30: times generated) that every sampler of the request updates -- the eager
        // first sample and the captured step alike -- so the decode-ahead loop needs no host round trip.  Greedy with a penalty = argmax of the adjusted logits.
        float min_p = 0.0f;                 ///< [0, 1): after top-k and top-p, drop the tokens less probable than min_p x the top token's probability; 0 = off
        float repetition_penalty = 1.0f;    ///< > 0: logits of prompt AND generated tokens divided (positive) or multiplied (negative) by it; 1 = off
        float presence_penalty = 0.0f;      ///< subtracted from the logit of every token generated so far in this request; 0 = off
        float frequency_penalty = 0.0f;     ///< times the number of times the token was generated, subtracted; 0 = off
        bool penalized() const noexcept { return repetition_penalty != 1.0f || presence_penalty != 0.0f || frequency_penalty != 0.0f; }
        bool filtered() const noexcept { return penalized() || min_p != 0.0f; }
    };
    /// the network's SamplingParams of a request's (the same fields); throws invalid_argument for filters the device library refuses
    template<typename TNet> typename TNet::SamplingParams networkSampling( const SamplingParams& s )
    {
        typename TNet::SamplingParams p;
        p.temperature = s.temperature; p.top_k = s.top_k; p.top_p = s.top_p;
        p.min_p = s.min_p; p.repetition_penalty = s.repetition_penalty; p.presence_penalty = s.presence_penalty; p.frequency_penalty = s.frequency_penalty;
        p.checkFilters( "GenerateParams::sampling" );
        return p;
    }
    /// proposes up to k tokens that may follow `history` (prompt + emitted tokens; its last element is the token about to be decoded)
    using DraftFunction = std::function<std::vector<int32_t>( std::span<const int32_t> history, int k )>;
    /// GenerateParams::on_logprobs: the log-probability of an emitted token under the model's distribution (softmax of the soft-capped logits: no temperature, no
    /// top-k / top-p) and the top_n most probable tokens, most probable first, ties to the lower id.  The spans are valid during the call only.
    struct TokenLogprobs
    {
        int row;                                 ///< generateBatch: the prompt's row; 0 otherwise
        int32_t token;
        float logprob;
        std::span<const int32_t> top_ids;
        std::span<const float> top_logprobs;
    };
    struct GenerateParams
    {
        std::optional<int> max_new_tokens;       ///< nullopt => run to EOS / the context bound
        SamplingParams sampling{};
        std::vector<int32_t> stop_tokens{};      ///< empty => the model's default stop set
        DraftFunction draft{};                   ///< speculative decode (GemmaModelConfig::withDraftTokens): the drafter; empty => promptLookupDraft
        bool speculative_sampling = false;       ///< a STOCHASTIC request on a withDraftTokens model takes the speculative loop too (coupled draws: the plain tokens)
        /// Sampling filters (sampling.min_p / .repetition_penalty / .presence_penalty / .frequency_penalty): a request with any of them set takes the plain loop, also
        /// on a withDraftTokens model and whatever speculative_sampling says (row t of a chain step would need the table plus the drafts 1 .. t: a follow-up);
        /// lastSpeculation() then reports zero chain steps.  They do not change the log-probabilities below: the samplers never touch the logits.
        /// token log-probabilities: the top-n to report (0 .. 20, 0 = the emitted token's alone); on_logprobs is then called immediately before on_token, for exactly
        /// the tokens on_token sees.  Computed on the device inside the decode step; tokens, status, generator state and prefix reuse are what they are without it.
        std::optional<int> logprobs;
        std::function<void( const TokenLogprobs& )> on_logprobs{};
        /// Logit bias, banned tokens, a closed answer set and min_tokens (Mila/TokenBias.h composes the four into ONE device table of vocab fp32 values that the
        /// samplers add to the capped logit; include/mila_cdna4.h: logit bias), all empty / 0 by default.  The table is written before the first sample; with
        /// min_tokens > 0 the stop tokens are forbidden until the step that produces sample index min_tokens (the first sampled token is index 0), in front of which
        /// the loop enqueues the restore in stream order -- one small launch, no host round trip, the captured step unchanged.  A request with any of them set takes
        /// the plain loop on a withDraftTokens model, as the sampling filters do, unless speculate_constrained (below) is set.  generateBatch shares one table among its rows.  Log-probabilities are those of the
        /// unbiased logits.  A request without them clears the network's bias.
        std::vector<std::pair<int32_t, float>> logit_bias{};      ///< id -> finite additive bias, an id at most once
        std::vector<int32_t> banned_tokens{};                     ///< never sampled (a ban wins over an allow)
        std::vector<int32_t> allowed_tokens{};                    ///< non-empty: only these may be sampled
        int min_tokens = 0;                                       ///< no stop token among the first min_tokens samples
        /// Grammar-constrained decoding (Mila/TokenAutomaton.h; include/mila_cdna4.h: token automaton): a deterministic automaton over token ids that says, state by
        /// state, which tokens may come next.  generate() validates it against the request's bias table (a reachable state that keeps no token with a transition and a
        /// finite bias is refused, with its number), uploads it and resets the state before the first sample; every step then ends with one launch that advances the
        /// state by the sampled token and rewrites the table the next sampler reads -- no logits readback, the captured step and the decode-ahead loop stay.  Stop
        /// tokens are ordinary tokens of the automaton.  min_tokens > 0 beside an automaton is refused (a chain of states says the same).  A constrained request takes
        /// the plain loop on a withDraftTokens model unless speculate_constrained (below) is set; generateBatch refuses one.  Log-probabilities stay those of the unconstrained logits.  A request without one
        /// clears the network's.  lastAutomatonState() reports where the request ended.
        std::shared_ptr<const TokenAutomaton> automaton{};
        /// Constrained speculative decode (a withDraftTokens model; greedy, or stochastic with speculative_sampling; no penalties and no min-p): a request with a bias
        /// table and / or an automaton takes the speculative loop instead of the plain one.  The chain step's tail reads row t's table (include/mila_cdna4.h: the
        /// constrained chain step), and the drafter starts with the tokens the automaton FORCES from the current state (TokenAutomaton::forcedTokens: states that
        /// allow one token -- drafted at no cost and accepted with certainty), then asks `draft` / the prompt lookup for the rest, cut at the first proposal the
        /// automaton forbids or whose bias is -inf.  The emitted tokens, the finish reason, the final state and the generator state are the plain loop's.
        /// Off by default: with it off such a request takes the plain loop, as it always did.
        bool speculate_constrained = false;
    };
    /// One row of GemmaModel::generateRequests: a prompt, its request and the seed of the row's generator
    struct BatchRequest
    {
        std::vector<int32_t> prompt;
        GenerateParams params{};
        uint64_t seed = 0;
    };
    /// the automaton of a request against its composed bias table (throws invalid_argument; touches no device)
    inline void checkRequestAutomaton( const GenerateParams& params, const TokenBiasPlan& bias_plan, dim_t vocab )
    {
        if ( !params.automaton ) return;
        if ( params.min_tokens > 0 ) throw std::invalid_argument( "GenerateParams: min_tokens > 0 together with an automaton (a chain of states expresses it)" );
        params.automaton->validate( vocab );
        params.automaton->checkLive( bias_plan );
    }
    /// the bias table of a request (throws invalid_argument for what composeTokenBias refuses); stop_ids: the request's effective stop set
    inline TokenBiasPlan composeRequestBias( const GenerateParams& params, const std::unordered_set<int32_t>& stop_ids, dim_t vocab )
    {
        TokenBiasRequest rq;
        rq.logit_bias = params.logit_bias; rq.banned_tokens = params.banned_tokens; rq.allowed_tokens = params.allowed_tokens;
        rq.min_tokens = params.min_tokens; rq.max_new_tokens = params.max_new_tokens;
        if ( params.min_tokens > 0 ) rq.stop_tokens.assign( stop_ids.begin(), stop_ids.end() );
        TokenBiasPlan plan = composeTokenBias( rq, vocab );
        if ( plan.restore_ids.size() > Compute::RocmTokenBias::kStage ) throw std::invalid_argument( "GenerateParams::min_tokens: a stop set of more than 1024 tokens" );
        return plan;
    }
    /// the request's table onto the network before the first sample (the restore list staged for commitTokenBiasUpdate()); a request without one clears the bias
    template<typename TNet> void applyRequestBias( TNet& net, const TokenBiasPlan& plan )
    {
        if ( !plan.active ) { net.clearTokenBias(); return; }
        net.setTokenBias( plan.fill, plan.ids.data(), plan.values.data(), plan.ids.size() );
        if ( plan.hasRestore() ) net.stageTokenBiasUpdate( plan.restore_ids.data(), plan.restore_values.data(), plan.restore_ids.size() );
    }
    /// throws invalid_argument for a GenerateParams::logprobs outside 0 .. min(20, vocabulary)
    inline void checkLogprobsRequest( const GenerateParams& params, dim_t vocab )
    {
        if ( params.logprobs && ( *params.logprobs < 0 || *params.logprobs > std::min<dim_t>( Compute::RocmTokenLogprobsOp::kMaxTop, vocab ) ) )
            throw std::invalid_argument( "GenerateParams::logprobs must be 0 .. min(20, vocabulary) (got " + std::to_string( *params.logprobs ) + ")" );
    }
    /// What generateRequests checks and composes for ONE row before anything is enqueued (host only: no device, no model).  sampling: the row's record -- a greedy
    /// request (top_k == 1 or temperature <= 0, generate()'s rule) is temperature 0 with the truncations off.
    struct RowRequestPlan
    {
        std::unordered_set<int32_t> stop_ids;
        TokenBiasPlan bias;
        SamplingParams sampling{};
        bool greedy = true;
        int max_new = 0;
    };
    /// every check generate() makes for the request, plus the rows rules (no speculative field; `logprobs` = the call's ONE top_n); throws invalid_argument with the
    /// row's number in the message.  default_stops: the model's stop set, taken when the request names none.  who: what the number counts (serveRequests: requests).
    inline RowRequestPlan planRowRequest( const BatchRequest& rq, const std::optional<int>& logprobs, int row, dim_t vocab, dim_t context, const std::unordered_set<int32_t>& default_stops,
                                          const char* who = "GemmaModel::generateRequests: row " )
    {
        try
        {
            if ( rq.prompt.empty() ) throw std::invalid_argument( "empty prompt" );
            if ( rq.prompt.size() > static_cast<size_t>( context ) ) throw std::invalid_argument( "the prompt exceeds the deployment context length" );
            for ( int32_t t : rq.prompt )
                if ( t < 0 || t >= vocab ) throw std::invalid_argument( "token id " + std::to_string( t ) + " outside the vocabulary" );
            const GenerateParams& p = rq.params;
            if ( p.speculative_sampling || p.speculate_constrained || p.draft )
                throw std::invalid_argument( "the speculative fields (speculative_sampling, speculate_constrained, draft) are not for a rows model: it has no chain" );
            if ( p.logprobs != logprobs ) throw std::invalid_argument( "logprobs differs from the call's: the step's log-probability launches have one top_n" );
            checkLogprobsRequest( p, vocab );
            RowRequestPlan pl;
            if ( p.stop_tokens.empty() ) pl.stop_ids = default_stops;
            else pl.stop_ids.insert( p.stop_tokens.begin(), p.stop_tokens.end() );
            pl.sampling = p.sampling;
            const SamplingParams& s = p.sampling;
            if ( !std::isfinite( s.temperature ) ) throw std::invalid_argument( "temperature is not finite" );
            if ( !std::isfinite( s.min_p ) || !std::isfinite( s.repetition_penalty ) || !std::isfinite( s.presence_penalty ) || !std::isfinite( s.frequency_penalty ) )
                throw std::invalid_argument( "a sampling filter is not finite" );
            if ( !( s.repetition_penalty > 0.0f ) ) throw std::invalid_argument( "repetition_penalty must be > 0" );
            if ( !( s.min_p >= 0.0f && s.min_p < 1.0f ) ) throw std::invalid_argument( "min_p outside [0, 1)" );
            pl.greedy = s.top_k == 1 || s.temperature <= 0.0f;
            if ( pl.greedy ) { pl.sampling.temperature = 0.0f; pl.sampling.top_k = 0; pl.sampling.top_p = 1.0f; }
            else if ( s.top_k < 0 || !( s.top_p > 0.0f ) ) throw std::invalid_argument( "need top_k >= 0, top_p > 0" );
            pl.max_new = p.max_new_tokens.value_or( static_cast<int>( context ) );
            pl.bias = composeRequestBias( p, pl.stop_ids, vocab );
            checkRequestAutomaton( p, pl.bias, vocab );
            return pl;
        }
        catch ( const std::invalid_argument& e ) { throw std::invalid_argument( who + std::to_string( row ) + ": " + e.what() ); }
    }
    /// host copies of the log-probabilities of up to four rows, and the callback over one of them
    struct TokenLogprobsRows
    {
        static constexpr int kMaxTop = Compute::RocmTokenLogprobsOp::kMaxTop;
        int top_n = 0;
        float logprob[ 4 ]{};
        int32_t top_ids[ 4 * kMaxTop ]{};
        float top_logprobs[ 4 * kMaxTop ]{};
        /// rows 0 .. rows - 1 of the op's device outputs (synchronizes)
        void read( const Compute::RocmTokenLogprobsOp& op, int rows ) { op.read( rows, top_n, logprob, top_ids, top_logprobs ); }
        /// one row of the op's outputs (row 0 there) into row `b` here
        void readInto( const Compute::RocmTokenLogprobsOp& op, int b )
        {
            op.read( 1, top_n, logprob + b, top_ids + static_cast<size_t>( b ) * top_n, top_logprobs + static_cast<size_t>( b ) * top_n );
        }
        void report( const std::function<void( const TokenLogprobs& )>& cb, int out_row, int b, int32_t token ) const
        {
            if ( !cb ) return;
            const size_t n = static_cast<size_t>( top_n );
            cb( TokenLogprobs{ out_row, token, logprob[ b ], std::span<const int32_t>( top_ids + b * n, n ), std::span<const float>( top_logprobs + b * n, n ) } );
        }
    };

    /// The draw bookkeeping of speculative sampling, host only.  The plain stochastic loop takes one uniform per sampled token from the model's generator.  A chain
    /// step of T rows that starts after e sampled tokens verifies its drafts against the samples the plain loop would have taken for tokens e .. e + T - 1, so it
    /// needs the NEXT T uniforms without taking them: peekDraws.  Afterwards only the tokens that were really emitted count: consumeDraws( n ) leaves the generator
    /// where n plain draws leave it.
    inline float nextDraw( std::mt19937_64& rng ) { return std::uniform_real_distribution<float>( 0.0f, 1.0f )( rng ); }
    inline std::vector<float> peekDraws( const std::mt19937_64& rng, int n )
    {
        std::mt19937_64 ahead = rng;
        std::vector<float> r;
        for ( int i = 0; i < n; ++i ) r.push_back( nextDraw( ahead ) );
        return r;
    }
    inline void consumeDraws( std::mt19937_64& rng, int n ) { for ( int i = 0; i < n; ++i ) (void)nextDraw( rng ); }

    /// The default drafter, prompt lookup: for n = 3, 2, 1 take the LATEST earlier occurrence of the last n tokens of `history` (one that starts before the suffix
    /// itself does) and propose the up-to-k tokens that followed it; the first n with an occurrence decides, no occurrence at any n proposes nothing.  Pure host code.
    inline std::vector<int32_t> promptLookupDraft( std::span<const int32_t> history, int k )
    {
        const std::ptrdiff_t h = static_cast<std::ptrdiff_t>( history.size() );
        if ( k <= 0 ) return {};
        for ( std::ptrdiff_t n = 3; n >= 1; --n )
        {
            if ( h < n + 1 ) continue;
            for ( std::ptrdiff_t j = h - n - 1; j >= 0; --j )
            {
                bool same = true;
                for ( std::ptrdiff_t i = 0; i < n && same; ++i ) same = history[ static_cast<size_t>( j + i ) ] == history[ static_cast<size_t>( h - n + i ) ];
                if ( !same ) continue;
                const std::ptrdiff_t first = j + n, last = std::min<std::ptrdiff_t>( first + k, h );
                return std::vector<int32_t>( history.begin() + first, history.begin() + last );
            }
        }
        return {};
    }
    /// score(): `first` = the first token that is scored (1 .. n - 1; positions below first - 1 need no head); argmax = also report the greedy token of every scored
    /// position and its log-probability
    struct ScoreParams { dim_t first{ 1 }; bool argmax{ false }; };
    /// one entry per scored token first .. n - 1: entry j = log P( token first + j | tokens before it ); argmax / argmax_logprob are empty without ScoreParams::argmax;
    /// sum = the float64 sum of logprob on the host
    struct ScoreResult { std::vector<float> logprob; std::vector<int32_t> argmax; std::vector<float> argmax_logprob; double sum{ 0.0 }; };

    /// what the last speculative generate() of a withDraftTokens model did (greedy, or stochastic with GenerateParams::speculative_sampling): decode steps in all,
    /// those that were chain steps, the drafter's tokens those carried (padding not counted) and how many of them were accepted
    /// forced / forced_accepted (GenerateParams::speculate_constrained): the drafted tokens that the automaton forced, and how many of those were accepted
    struct SpeculationStats { uint64_t steps = 0, chain_steps = 0, drafted = 0, accepted = 0, forced = 0, forced_accepted = 0; };

    struct GemmaModelConfig
    {
        GemmaModelConfig() = default;
        explicit GemmaModelConfig( dim_t context_length ) { withContextLength( context_length ); }
        GemmaModelConfig& withContextLength( dim_t n )
        {
            if ( n <= 0 ) throw std::invalid_argument( "LanguageModelConfig: context_length must be greater than zero" );
            context_length_ = n;
            return *this;
        }
        GemmaModelConfig& withWeightQuantization( WeightQuantization wq ) { weight_quantization_ = wq; return *this; }
        GemmaModelConfig& withKvCacheCompression( KvCacheCompression kv ) { kv_cache_compression_ = kv; return *this; }
        /// MI355X deployment knobs (no reference counterpart: a 12 GB card always chunks and always bounds the ring)
        GemmaModelConfig& withPrefillChunk( dim_t chunk ) { prefill_chunk_ = chunk; return *this; }          ///< 0 = min(context, 2048)
        GemmaModelConfig& withBoundedLocalKv( bool on ) { bounded_local_kv_ = on; return *this; }            ///< SlidingWindowKvCache on the sliding-window layers
        GemmaModelConfig& withMaxBatch( dim_t n ) { max_batch_ = n; return *this; }                           ///< GemmaConfig::max_batch: sequences per decode step (generateBatch), 1 .. 4
        dim_t maxBatch() const noexcept { return max_batch_; }
        /// GemmaConfig::draft_tokens (0 .. 3): greedy generate() verifies up to k drafted tokens per step on the chain step and emits up to k + 1 tokens per step --
        /// token for token the plain greedy output.  A plain step loop (one sync per step, no decode-ahead, as generateBatch).  Stochastic requests keep the plain
        /// path unless GenerateParams::speculative_sampling is set: then a draft is verified against the SAMPLE the plain loop would have taken at that token (the
        /// same uniform draw), so the output is token for token the plain stochastic output for the same seed, and a deterministic draft d is accepted with
        /// probability p( d ).
        GemmaModelConfig& withDraftTokens( dim_t k ) { draft_tokens_ = k; return *this; }
        dim_t draftTokens() const noexcept { return draft_tokens_; }
        GemmaModelConfig& withKvFp8( bool on ) { kv_fp8_ = on; return *this; }                               ///< PerChannelKvFp8<> on every layer (GemmaConfig::kv_fp8), under any weight policy
        /// GemmaConfig::kv_fp8_rows: the FP8 KV cache (implied) on a model of max_batch 1 .. 4 -- generateBatch / generateRequests / serveRequests over FP8 rows
        GemmaModelConfig& withKvFp8Rows( bool on ) { kv_fp8_rows_ = on; return *this; }
        bool kvFp8Rows() const noexcept { return kv_fp8_rows_; }
        /// GemmaConfig::bounded_local_kv_rows: rings on the sliding-window layers (bounded_local_kv, implied) on a model of max_batch 1 .. 4 -- generateBatch /
        /// generateRequests / serveRequests over rows that keep window + chunk - 1 positions per sliding-window layer; forks copy the live band
        GemmaModelConfig& withBoundedLocalKvRows( bool on ) { bounded_local_kv_rows_ = on; return *this; }
        bool boundedLocalKvRows() const noexcept { return bounded_local_kv_rows_; }
        dim_t getContextLength() const noexcept { return context_length_; }
        WeightQuantization getWeightQuantization() const noexcept { return weight_quantization_; }
        KvCacheCompression getKvCacheCompression() const noexcept { return kv_cache_compression_; }
        dim_t getPrefillChunk() const noexcept { return prefill_chunk_ > 0 ? std::min( prefill_chunk_, context_length_ ) : std::min<dim_t>( context_length_, 2048 ); }
        bool boundedLocalKv() const noexcept { return bounded_local_kv_; }
        bool kvFp8() const noexcept { return kv_fp8_; }
    private:
        dim_t context_length_{ 0 }, prefill_chunk_{ 0 }, max_batch_{ 1 }, draft_tokens_{ 0 };
        WeightQuantization weight_quantization_{ WeightQuantization::None };
        KvCacheCompression kv_cache_compression_{ KvCacheCompression::None };
        bool bounded_local_kv_{ false }, kv_fp8_{ false }, kv_fp8_rows_{ false }, bounded_local_kv_rows_{ false };
    };

    /// Models/QuantizationDispatch.ixx: the runtime deployment choice picks the compile-time policy
    template<TensorDataType TPrecision, typename TResult, typename TAction>
    TResult dispatchWeightQuantization( WeightQuantization wq, KvCacheCompression kv, std::string_view caller, TAction&& action )
    {
        static_assert( TPrecision == TensorDataType::BF16, "the CDNA4 backend computes in BF16" );
        switch ( wq )
        {
            case WeightQuantization::FP4: return action.template operator()<Quant::Weight::PerGroupFp4<128>>();
            case WeightQuantization::FP8: return action.template operator()<Quant::Weight::PerChannelFp8<>>();
            case WeightQuantization::None:
            default:
                if ( kv == KvCacheCompression::FP8 ) throw std::runtime_error( std::string( caller ) + ": FP8 KV cache compression is not yet supported" );
                return action.template operator()<Quant::Weight::NoWeightQuant>();
        }
    }

    template<DeviceType TDeviceType, TensorDataType TPrecision>
    class GemmaModel
    {
        static_assert( TDeviceType == DeviceType::Rocm && TPrecision == TensorDataType::BF16, "GemmaModel<Rocm, BF16>" );
    public:
        template<typename P> using Net = GemmaTransformer<P>;
        using Network = std::variant<std::unique_ptr<Net<Quant::Weight::NoWeightQuant>>, std::unique_ptr<Net<Quant::Weight::PerChannelFp8<>>>,
                                     std::unique_ptr<Net<Quant::Weight::PerGroupFp4<128>>>>;
        using TokenTensor = Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>;
        static constexpr int32_t kEosToken = 1, kEndOfTurnToken = 106;

        GemmaModel( const GemmaModel& ) = delete;
        GemmaModel& operator=( const GemmaModel& ) = delete;
        ~GemmaModel()
        {
            if ( ring_host_ ) (void)hipHostFree( ring_host_ );
            if ( draws_host_ ) (void)hipHostFree( draws_host_ );
            if ( lp_ring_host_ ) (void)hipHostFree( lp_ring_host_ );
            if ( row_draws_host_ ) (void)hipHostFree( row_draws_host_ );
        }

        /// every architectural parameter comes from the artifact's metadata; `model_config` carries the deployment decisions
        static std::unique_ptr<GemmaModel> fromPretrained( const std::string& path, const GemmaModelConfig& model_config, DeviceId device_id = Compute::Device::Rocm( 0 ) )
        {
            if ( device_id.type != TDeviceType ) throw std::invalid_argument( "GemmaModel::fromPretrained: device type mismatch" );
            if ( model_config.getContextLength() == 0 ) throw std::invalid_argument( "GemmaModel::fromPretrained: context_length must be greater than zero" );
            return dispatchWeightQuantization<TPrecision, std::unique_ptr<GemmaModel>>( model_config.getWeightQuantization(), model_config.getKvCacheCompression(), "GemmaModel::fromPretrained",
                [&]<typename TWeightQuantization>()
                {
                    Serialization::PretrainedModelReader reader( path );
                    const auto& md = reader.getPretrainedMetadata();
                    const std::string& artifact = reader.getWeightQuantization();
                    const std::string requested = weightQuantizationName( model_config.getWeightQuantization() );
                    if ( !artifact.empty() && artifact != requested )
                        throw std::runtime_error( "GemmaModel::fromPretrained: artifact '" + path + "' is pre-quantized as '" + artifact + "' but this load requested '" + requested + "'" );
                    if ( reader.metadataJSON().empty() ) throw std::runtime_error( "GemmaModel::fromPretrained: artifact '" + path + "' carries no mila_config metadata" );
                    GemmaConfig cfg = configFromMetadata( md );
                    if ( md.max_seq_length != 0 && model_config.getContextLength() > static_cast<dim_t>( md.max_seq_length ) )
                        throw std::invalid_argument( "GemmaModel::fromPretrained: context_length " + std::to_string( model_config.getContextLength() ) + " exceeds trained max_seq_len " + std::to_string( md.max_seq_length ) );
                    cfg.bounded_local_kv = model_config.boundedLocalKv();
                    cfg.kv_fp8 = model_config.kvFp8();
                    cfg.kv_fp8_rows = model_config.kvFp8Rows();
                    cfg.bounded_local_kv_rows = model_config.boundedLocalKvRows();
                    cfg.max_batch = model_config.maxBatch();
                    cfg.draft_tokens = model_config.draftTokens();
                    auto net = std::make_unique<Net<TWeightQuantization>>( cfg, model_config.getContextLength(), model_config.getPrefillChunk(), device_id );
                    net->loadPretrained( path );
                    return std::unique_ptr<GemmaModel>( new GemmaModel( Network( std::move( net ) ), cfg, model_config, md ) );
                } );
        }
        /// the same model over synthetic parameters (no artifact offline): tests and benchmarks
        static std::unique_ptr<GemmaModel> fromSynthetic( const GemmaConfig& network_config, const GemmaModelConfig& model_config, uint64_t seed,
                                                          const typename Net<Quant::Weight::NoWeightQuant>::SyntheticProfile& profile = {}, DeviceId device_id = Compute::Device::Rocm( 0 ) )
        {
            return dispatchWeightQuantization<TPrecision, std::unique_ptr<GemmaModel>>( model_config.getWeightQuantization(), model_config.getKvCacheCompression(), "GemmaModel::fromSynthetic",
                [&]<typename TWeightQuantization>()
                {
                    GemmaConfig cfg = network_config;
                    cfg.bounded_local_kv = model_config.boundedLocalKv();
                    cfg.kv_fp8 = model_config.kvFp8();
                    cfg.kv_fp8_rows = model_config.kvFp8Rows();
                    cfg.bounded_local_kv_rows = model_config.boundedLocalKvRows();
                    cfg.max_batch = model_config.maxBatch();
                    cfg.draft_tokens = model_config.draftTokens();
                    auto net = std::make_unique<Net<TWeightQuantization>>( cfg, model_config.getContextLength(), model_config.getPrefillChunk(), device_id );
                    typename Net<TWeightQuantization>::SyntheticProfile p;
                    p.linear_gain = profile.linear_gain; p.qk_norm_center = profile.qk_norm_center; p.post_norm_center = profile.post_norm_center; p.layer_scalar = profile.layer_scalar; p.table_gain = profile.table_gain;
                    net->initSynthetic( seed, p );
                    return std::unique_ptr<GemmaModel>( new GemmaModel( Network( std::move( net ) ), cfg, model_config, Serialization::PretrainedMetadata{} ) );
                } );
        }
        static GemmaConfig configFromMetadata( const Serialization::PretrainedMetadata& md )
        {
            GemmaConfig c;
            auto take = [&]( dim_t& dst, uint32_t v ) { if ( v != 0 ) dst = static_cast<dim_t>( v ); };
            take( c.vocab_size, md.vocab_size ); take( c.embedding_dim, md.embedding_dim ); take( c.num_layers, md.num_layers ); take( c.num_heads, md.num_heads );
            take( c.num_kv_heads, md.num_kv_heads ); take( c.head_dim, md.head_dim ); take( c.hidden_dim, md.hidden_dim ); take( c.global_head_dim, md.global_head_dim );
            take( c.num_global_kv_heads, md.num_global_kv_heads ); take( c.window, md.window ); take( c.sliding_window_pattern, md.sliding_window_pattern );
            take( c.global_rotary_dim, md.global_rotary_dim );
            if ( md.norm_epsilon > 0.0f ) c.rms_norm_eps = md.norm_epsilon;
            if ( md.rope_theta_local > 0.0f ) c.rope_theta_local = md.rope_theta_local;
            if ( md.rope_theta_global > 0.0f ) c.rope_theta_global = md.rope_theta_global;
            c.final_logit_softcapping = md.final_logit_softcapping;
            c.validate();
            return c;
        }

        const GemmaConfig& getNetworkConfig() const noexcept { return network_config_; }
        const GemmaModelConfig& getModelConfig() const noexcept { return model_config_; }
        dim_t contextLength() const noexcept { return model_config_.getContextLength(); }
        dim_t vocabSize() const noexcept { return network_config_.vocab_size; }
        int32_t eosToken() const noexcept { return kEosToken; }
        std::unordered_set<int32_t> stopTokens() const { return { kEosToken, kEndOfTurnToken }; }
        float finalLogitSoftcap() const noexcept { return network_config_.final_logit_softcapping; }
        void seedSampler( uint64_t seed ) { rng_.seed( seed ); }
        /// tokens the KV caches currently hold (prompt + everything decoded into them), the key of the prefix reuse
        const std::vector<int32_t>& kvTokenHistory() const noexcept { return kv_token_history_; }
        /// prompt tokens the last generate() did NOT have to prefill
        dim_t lastReusedPrefix() const noexcept { return last_reuse_; }
        /// the speculative loop's counters of the last generate() (all zero on a model without draft tokens, or after a stochastic request without
        /// GenerateParams::speculative_sampling)
        const SpeculationStats& lastSpeculation() const noexcept { return last_speculation_; }
        /// the automaton state the last generate() ended in: the state after its last sample, a stop token included (nullopt: the request had no automaton)
        std::optional<int32_t> lastAutomatonState() const noexcept { return last_automaton_state_; }
        Network& network() noexcept { return network_; }

        /// prefill + decode; on_token is called for every generated token except a stop token
        [[nodiscard]] GenerateStatus generate( std::span<const int32_t> prompt_tokens, const std::function<void( int32_t )>& on_token, const GenerateParams& params = {},
                                               const std::atomic<bool>* stop = nullptr )
        {
            return std::visit( [&]( auto& net )
            {
                prefix_cache_.clear();      // (row 0's caches are written: the rows' claims end here)
                try { return onGenerating( *net, prompt_tokens, on_token, params, stop ); }
                catch ( const std::invalid_argument& ) { throw; }      // the request checks: nothing was enqueued, the caches are untouched
                catch ( ... )
                {
                    // a replay may still be in flight (awaitSampledToken's timeout, a throwing on_token): drain it before the caller sees the exception,
                    // and drop the reuse key -- what the in-flight step wrote is not in the history
                    try { net->context()->synchronize(); } catch ( ... ) {}
                    kv_token_history_.clear();
                    throw;
                }
            }, network_ );
        }

        /// Score a token sequence: the log-probability of every token first .. n - 1 given the tokens before it, from the prefill itself (GemmaTransformer::
        /// prefillScored: the logits are never formed).  Chunked by the model's prefill chunk: the target of a chunk's last row is the next chunk's first token; the
        /// sequence's last row has no target and is not scored.  KV prefix reuse as generate()'s, except that positions below first - 1 need no head, so
        /// reuse = min( common prefix with kvTokenHistory(), first - 1 ): scoring many continuations of one context prefills the context once.  Afterwards the history
        /// holds all n tokens: a generate() on the same tokens re-prefills only the last position (echo = score() + generate() at the cost of one prefill).
        /// Failures as generate()'s: invalid_argument before anything is enqueued (n < 2, n beyond the context length, first outside 1 .. n - 1, a token id outside
        /// the vocabulary); anything else drains the stream and clears the history.
        [[nodiscard]] ScoreResult score( std::span<const int32_t> tokens, const ScoreParams& params = {} )
        {
            return std::visit( [&]( auto& net )
            {
                prefix_cache_.clear();
                try { return onScoring( *net, tokens, params ); }
                catch ( const std::invalid_argument& ) { throw; }
                catch ( ... )
                {
                    try { net->context()->synchronize(); } catch ( ... ) {}
                    kv_token_history_.clear();
                    throw;
                }
            }, network_ );
        }

        /// generate() for up to max_batch independent requests at once (GemmaModelConfig::withMaxBatch > 1): prompt b runs in row b, each at its own position, the
        /// weights streamed once per step for all of them.  on_token( row, token ) as generate()'s on_token; one GenerateStatus per prompt, by generate()'s rules (stop
        /// token, max_new_tokens, context limit -- the parameters are shared by the rows).  A plain step loop: every step replays the rows graph, reads the rows' tokens
        /// back and retires finished rows by clearing their active word (a retired row stays frozen); no decode-ahead yet.  Greedy: the tokens generate() gives for each
        /// prompt alone.  Stochastic: row b samples with the radix sampler from its own generator seeded seed + b, so a one-prompt batch with seed s gives generate()'s
        /// tokens after seedSampler( s ); the sampler runs inside the rows graph, over all rows in one pipeline, at the draws the host writes before each replay.
        /// The prompt-prefix reuse of generate() is dropped: the history is cleared.
        [[nodiscard]] std::vector<GenerateStatus> generateBatch( std::span<const std::vector<int32_t>> prompts, const std::function<void( int, int32_t )>& on_token,
                                                                 const GenerateParams& params = {}, uint64_t seed = 0 )
        {
            return std::visit( [&]( auto& net )
            {
                kv_token_history_.clear();      // row 0's caches are overwritten; whatever happens below, nothing is left to reuse
                prefix_cache_.clear();
                last_reuse_ = 0;
                try { return onGeneratingBatch( *net, prompts, on_token, params, seed ); }
                catch ( const std::invalid_argument& ) { throw; }
                catch ( ... ) { try { net->context()->synchronize(); } catch ( ... ) {} throw; }
            }, network_ );
        }

        /// generateBatch for requests that do NOT agree: row b runs requests[ b ] -- its own sampling (all seven fields; greedy and stochastic rows mix), stop set,
        /// max_new_tokens, logit_bias / banned_tokens / allowed_tokens / min_tokens and automaton -- with its own generator seeded requests[ b ].seed.  THE CONTRACT:
        /// row b gives, token for token, what generate() gives for request b alone on a one-sequence model of the same weights after seedSampler( seed_b ) -- tokens,
        /// finish reason, log-probability bits and the final automaton state -- whatever the other rows carry (the rows step's invariance, with its one documented
        /// limit: the unwindowed layers' live-length bucket follows the batch's longest row).  logprobs / on_logprobs: ONE n for the call (the step's two
        /// log-probability launches have one top_n), so differing values are refused; the callback reported is each row's own.  The speculative fields
        /// (speculative_sampling, speculate_constrained, draft) are refused: a rows model has no chain.  Every request check happens before anything is enqueued, with
        /// the row's number in the message.  final_states (may be null): row b's automaton state after its last sample, nullopt for a row without one.
        /// The sampler parameters live in device memory (GemmaTransformer::setRowsRequests): a second call with other parameters of the same classes replays the
        /// captured rows graph.  generateBatch keeps its contract; this is an entry beside it.
        [[nodiscard]] std::vector<GenerateStatus> generateRequests( std::span<const BatchRequest> requests, const std::function<void( int, int32_t )>& on_token,
                                                                    std::vector<std::optional<int32_t>>* final_states = nullptr )
        {
            return std::visit( [&]( auto& net )
            {
                prefix_cache_.clear();
                try
                {
                    auto status = onGeneratingRequests( *net, requests, on_token, final_states );
                    net->clearRowsRequests();
                    return status;
                }
                catch ( const std::invalid_argument& ) { net->clearRowsRequests(); throw; }
                catch ( ... ) { try { net->context()->synchronize(); } catch ( ... ) {} net->clearRowsRequests(); kv_token_history_.clear(); throw; }
            }, network_ );
        }

        /// What a serveRequests call did: the rows steps it replayed, the prefills it ran and their tokens, the rows that took a fork in place of a prefill, the
        /// rows-graph captures during the call, and per request the row it ran in and the number of steps replayed before its admission.  The four times are host
        /// wall-clock sums over the call's admissions (every phase ends in a synchronize of its own): the rows' setters, the prefills, the forks, and the first
        /// samples with their readback
        struct ServeStats
        {
            int64_t steps = 0, prefills = 0, prefill_tokens = 0, forks = 0, captures = 0;
            double setters_ms = 0.0, prefill_ms = 0.0, fork_ms = 0.0, first_sample_ms = 0.0;
            std::vector<int> row;
            std::vector<int64_t> admitted_at;
            // with ServeParams::prefix_cache (otherwise empty / zero).  Per request: the prompt positions it did not prefill and the row they came from (-1: none, its
            // own row: in place; a request forked whole by the identical-prompt rule: its whole prompt and that row).  Totals: the forkRowPrefix calls and the
            // admissions that reused their own row in place.  prefill_tokens counts the tokens actually prefilled
            std::vector<int64_t> reused_tokens;
            std::vector<int> donor_row;
            int64_t prefix_forks = 0, prefix_in_place = 0;
        };
        /// serveRequests' options.  prefix_cache: reuse cached KV prefixes across requests and calls (below); min_prefix: the shortest prefix worth reusing (>= 1)
        struct ServeParams
        {
            bool prefix_cache = false;
            int min_prefix = 1;
        };
        /// generateRequests for ANY number of requests (>= 1) on a withMaxBatch( R > 1 ) model: a queue in front of the rows step.  Requests are admitted in FIFO
        /// order, each into the lowest free row (Mila/RequestQueue.h holds the rule): the first min( n, R ) at the start, and after every step's readback each retired
        /// row goes to the next waiting request before the next replay.  Admission runs what generateRequests runs per row, in its order -- resetRow, the automaton or
        /// its clear, the bias table and its staged restore, setRowRequest, prefillRow, resetTokenTable, the first sample at the first draw of the request's OWN
        /// generator (mt19937_64( seed )), its log-probability record, setRowActive -- and delivers the first token at once: a stop token there ends the request with
        /// zero tokens and frees the row in the same round.  Requests admitted in the same round with an identical prompt share ONE prefill: the others take
        /// GemmaTransformer::forkRow from that row, then their own table reset and first sample; nothing else is shared.  A row that has stepped is never forked from.
        /// THE CONTRACT is generateRequests': request i gives, token for token, what generate() gives for it alone on a one-sequence model of the same weights after
        /// seedSampler( seed_i ) -- tokens, finish reason, log-probability bits, final automaton state -- whatever the other requests are, whichever row it landed
        /// in, whenever it was admitted, prefilled or forked (same limit: the unwindowed layers' live-length bucket follows the longest live row).
        /// on_token( request, token ) / on_finish( request, status ) (once per request) / on_logprobs report the REQUEST's number.  logprobs: one n for the call.
        /// Every request is checked before anything is enqueued, with its number in the message.  Not here: requests arriving during the call, cancellation,
        /// priorities, decode-ahead; prefixes shorter than a whole prompt are the ServeParams overload below.
        [[nodiscard]] std::vector<GenerateStatus> serveRequests( std::span<const BatchRequest> requests, const std::function<void( int, int32_t )>& on_token,
                                                                 const std::function<void( int, GenerateStatus )>& on_finish = {},
                                                                 std::vector<std::optional<int32_t>>* final_states = nullptr, ServeStats* stats = nullptr )
        {
            return serveRequests( requests, on_token, ServeParams{}, on_finish, final_states, stats );
        }
        /// serveRequests with options.  ServeParams{} is the call above, launch for launch.  prefix_cache = true: THE PREFIX CACHE (Mila/PrefixCache.h holds the rule).
        /// Every row has a claim -- the tokens whose KV its caches hold at [0, n) -- that outlives its request: a retired row keeps it until the row is written.  The
        /// cache work of a round runs admission by admission, in the queue's order: the identical-prompt rule first and unchanged (forkRow, logits and all, no
        /// prefill); otherwise plan() finds the longest prefix L <= len - 1 of the prompt that any row holds -- live, retired, or the request's own row -- and the
        /// admission is forkRowPrefix( donor, row, L ) (none when the donor is the own row: in place), then prefillRow( row, prompt[ L: ], len - L, L ), whose chunks
        /// are the ones generate() cuts from its reuse.  After every step each live row's claim grows by the token it was fed.  The claims live in the model: a later
        /// serveRequests( prefix_cache ) reuses them; generate, generateBatch, generateRequests, score and a serveRequests without the flag clear them on entry, and so
        /// does any exception out of a serving call (clearPrefixCache(): by hand).
        /// THE CONTRACT: request i, admitted with reuse L from a chain of donors, gives what generate() gives for it on a one-sequence model on which the requests of
        /// that chain ran before it, in order, generate() itself reusing L positions -- a prefilled suffix takes another GEMM form than a whole prompt (fp8 weights:
        /// other bits), so the reuse path is the oracle, not a cold prefill.  min_prefix < 1 is refused before anything is enqueued.  Not here: copying only a
        /// windowed layer's live band, choosing the free row by best match, eviction beyond "a written row loses its claim".
        [[nodiscard]] std::vector<GenerateStatus> serveRequests( std::span<const BatchRequest> requests, const std::function<void( int, int32_t )>& on_token, const ServeParams& serve,
                                                                 const std::function<void( int, GenerateStatus )>& on_finish = {},
                                                                 std::vector<std::optional<int32_t>>* final_states = nullptr, ServeStats* stats = nullptr )
        {
            return std::visit( [&]( auto& net )
            {
                try
                {
                    auto status = onServingRequests( *net, requests, on_token, serve, on_finish, final_states, stats );
                    net->clearRowsRequests();
                    return status;
                }
                catch ( const std::invalid_argument& ) { net->clearRowsRequests(); prefix_cache_.clear(); throw; }
                catch ( ... ) { try { net->context()->synchronize(); } catch ( ... ) {} net->clearRowsRequests(); kv_token_history_.clear(); prefix_cache_.clear(); throw; }
            }, network_ );
        }
        /// forget what the rows hold: the next serveRequests( prefix_cache ) prefills every prompt whole
        void clearPrefixCache() noexcept { prefix_cache_.clear(); }
        /// per row of the model: the number of cache positions the prefix cache knows the tokens of
        std::vector<int64_t> prefixCacheLengths() const
        {
            const int R = std::visit( []( const auto& net ) { return static_cast<int>( net->maxBatch() ); }, network_ );
            std::vector<int64_t> out;
            for ( int r = 0; r < std::min( R, PrefixCache::kMaxRows ); ++r ) out.push_back( static_cast<int64_t>( prefix_cache_.claim( r ).size() ) );
            return out;
        }

    private:
        template<typename TNet>
        std::vector<GenerateStatus> onServingRequests( TNet& net, std::span<const BatchRequest> requests, const std::function<void( int, int32_t )>& on_token,
                                                       const ServeParams& serve, const std::function<void( int, GenerateStatus )>& on_finish,
                                                       std::vector<std::optional<int32_t>>* final_states, ServeStats* stats )
        {
            Compute::TraceRange tr( "GemmaModel.serveRequests" );
            const size_t n = requests.size();
            const int R = static_cast<int>( net.maxBatch() );
            if ( R < 2 ) throw std::invalid_argument( "GemmaModel::serveRequests: the model was built for one sequence (GemmaModelConfig::withMaxBatch)" );
            if ( n < 1 ) throw std::invalid_argument( "GemmaModel::serveRequests: no request" );
            if ( serve.min_prefix < 1 ) throw std::invalid_argument( "GemmaModel::serveRequests: min_prefix " + std::to_string( serve.min_prefix ) + " (>= 1)" );
            const bool cached = serve.prefix_cache;
            std::vector<RowRequestPlan> plan;
            std::vector<typename TNet::SamplingParams> sp;
            std::vector<std::span<const int32_t>> prompts;
            for ( size_t q = 0; q < n; ++q )
            {
                plan.push_back( planRowRequest( requests[ q ], requests[ 0 ].params.logprobs, static_cast<int>( q ), vocabSize(), contextLength(), stopTokens(), "GemmaModel::serveRequests: request " ) );
                sp.push_back( networkSampling<TNet>( plan.back().sampling ) );
                prompts.emplace_back( requests[ q ].prompt );
            }
            RequestQueue queue( R, promptClasses( prompts ) );
            // ---- nothing was enqueued so far
            kv_token_history_.clear();      // row 0's caches are overwritten: nothing is left to reuse
            last_reuse_ = 0;
            if ( !cached ) prefix_cache_.clear();      // this call writes rows and keeps no account of it
            const std::optional<int> logprobs = requests[ 0 ].params.logprobs;
            auto* ctx = net.context();
            net.clearTokenAutomaton();
            net.clearRowsRequests();      // every row vacant until its first admission (setRowRequest)
            // a row between requests: position 0 and inactive -- except that under the prefix cache a row keeps its position word until it is written (the word says
            // how far its caches were written, which is what forkRowPrefix checks a donor against; an inactive row's position is read by nothing else)
            auto vacate = [&]( int b ) { if ( cached ) net.setRowActive( b, false ); else net.resetRow( b ); };
            for ( int b = static_cast<int>( std::min<size_t>( n, static_cast<size_t>( R ) ) ); b < R; ++b )      // a row no request will enter at the start: as generateRequests leaves it
            {
                vacate( b );
                net.clearRowTokenAutomaton( b );
                net.clearRowTokenBias( b );
            }
            net.setStepLogprobs( logprobs );
            const size_t captures0 = net.graphRowsCaptureCount();
            ServeStats st;
            st.row.assign( n, -1 );
            st.admitted_at.assign( n, -1 );
            if ( cached ) { st.reused_tokens.assign( n, 0 ); st.donor_row.assign( n, -1 ); }
            std::vector<int32_t> last_token( static_cast<size_t>( R ), 0 );      // per row: its latest sample, which the next step feeds (the prefix cache's fed())
            TokenLogprobsRows lp;
            lp.top_n = logprobs.value_or( 0 );
            std::vector<GenerateStatus> status( n, GenerateStatus::Success );
            if ( final_states ) final_states->assign( n, std::nullopt );
            // per ROW: the generator, position, emitted tokens and sample index of the request the row holds (rows are not in lockstep: all counted from the admission)
            std::vector<std::mt19937_64> rng( static_cast<size_t>( R ) );
            std::vector<dim_t> position( static_cast<size_t>( R ), 0 );
            std::vector<int> emitted( static_cast<size_t>( R ), 0 ), samples( static_cast<size_t>( R ), 0 );
            auto draw = [&]( int b ) { return std::uniform_real_distribution<float>( 0.0f, 1.0f )( rng[ static_cast<size_t>( b ) ] ); };
            auto finish = [&]( int b, GenerateStatus s )
            {
                const int q = queue.requestOf( b );
                status[ static_cast<size_t>( q ) ] = s;
                if ( final_states ) ( *final_states )[ static_cast<size_t>( q ) ] = net.rowTokenAutomatonState( b );      // before the row is handed on
                net.setRowActive( b, false );
                queue.retire( b );
                if ( on_finish ) on_finish( q, s );
            };
            // generateRequests' rules in its order: stop token, max_new_tokens, context.  true: the request has ended and its row is free
            auto deliver = [&]( int b, int32_t token )
            {
                const int q = queue.requestOf( b );
                const size_t i = static_cast<size_t>( q );
                if ( plan[ i ].stop_ids.contains( token ) ) { finish( b, GenerateStatus::Success ); return true; }
                if ( logprobs ) lp.report( requests[ i ].params.on_logprobs, q, b, token );
                on_token( q, token );
                ++emitted[ static_cast<size_t>( b ) ];
                if ( emitted[ static_cast<size_t>( b ) ] >= plan[ i ].max_new ) { finish( b, GenerateStatus::MaxNewTokensReached ); return true; }
                if ( position[ static_cast<size_t>( b ) ] >= contextLength() ) { finish( b, GenerateStatus::ContextOverflow ); return true; }
                return false;
            };
            using Clock = std::chrono::steady_clock;
            auto since = []( Clock::time_point t0 ) { return std::chrono::duration<double, std::milli>( Clock::now() - t0 ).count(); };
            auto admitRound = [&]
            {
                for ( auto wave = queue.admit(); !wave.empty(); wave = queue.admit() )
                {
                    auto t0 = Clock::now();
                    for ( const auto& a : wave )      // the row's setters, in generateRequests' order
                    {
                        const int b = a.row;
                        const size_t i = static_cast<size_t>( a.request );
                        vacate( b );
                        const GenerateParams& p = requests[ i ].params;
                        // the automaton first: a row with one keeps its bias in the table the automaton composes from
                        if ( p.automaton ) net.setRowTokenAutomaton( b, *p.automaton ); else net.clearRowTokenAutomaton( b );
                        const TokenBiasPlan& bp = plan[ i ].bias;
                        if ( bp.active )
                        {
                            net.setRowTokenBias( b, bp.fill, bp.ids.data(), bp.values.data(), bp.ids.size() );
                            if ( bp.hasRestore() ) net.stageRowTokenBiasUpdate( b, bp.restore_ids.data(), bp.restore_values.data(), bp.restore_ids.size() );
                        }
                        else net.clearRowTokenBias( b );
                        net.setRowRequest( b, sp[ i ], row_draws_dev_ );
                        rng[ static_cast<size_t>( b ) ] = std::mt19937_64( requests[ i ].seed );
                        emitted[ static_cast<size_t>( b ) ] = 0;
                        samples[ static_cast<size_t>( b ) ] = 0;
                        st.row[ i ] = b;
                        st.admitted_at[ i ] = queue.steps();
                    }
                    st.setters_ms += since( t0 );
                    unsigned filled = 0;      // rows of this wave whose caches, logits and position are in place
                    auto forkFrom = [&]( int src, dim_t len )      // ONE fork for every row of the wave that shares row src's prefill
                    {
                        unsigned mask = 0;
                        for ( const auto& m : wave ) if ( m.fork_from == src && !( ( filled >> m.row ) & 1u ) ) mask |= 1u << m.row;
                        if ( !mask ) return;
                        const auto f0 = Clock::now();
                        net.forkRow( src, mask, len );
                        ctx->synchronize();
                        st.fork_ms += since( f0 );
                        filled |= mask;
                        st.forks += std::popcount( mask );
                    };
                    for ( const auto& a : wave )
                    {
                        const auto& prompt = requests[ static_cast<size_t>( a.request ) ].prompt;
                        const dim_t len = static_cast<dim_t>( prompt.size() );
                        if ( cached )      // one admission after the other: each sees the claims as the ones before it left them (Mila/PrefixCache.h)
                        {
                            const size_t i = static_cast<size_t>( a.request );
                            const std::span<const int32_t> whole( prompt );
                            if ( a.fork_from >= 0 )      // the identical-prompt rule, unchanged: a whole fork, logits and position included
                            {
                                const auto f0 = Clock::now();
                                prefix_cache_.beginWrite( a.row, 0 );
                                net.forkRow( a.fork_from, 1u << a.row, len );
                                ctx->synchronize();
                                prefix_cache_.adopt( a.row, whole );      // (a ring model's fork is the live band: the claim comes with its valid-from bound)
                                st.fork_ms += since( f0 );
                                ++st.forks;
                                st.reused_tokens[ i ] = len;
                                st.donor_row[ i ] = a.fork_from;
                                continue;
                            }
                            const PrefixCache::Plan pl = prefix_cache_.plan( a.row, whole, serve.min_prefix );
                            const dim_t L = static_cast<dim_t>( pl.reuse );
                            prefix_cache_.beginWrite( a.row, pl.donor == a.row ? static_cast<size_t>( L ) : 0 );      // before anything writes the row
                            if ( L > 0 && pl.donor != a.row )
                            {
                                const auto f0 = Clock::now();
                                net.forkRowPrefix( pl.donor, 1u << a.row, L );
                                ctx->synchronize();
                                prefix_cache_.adopt( a.row, whole.first( static_cast<size_t>( L ) ) );
                                st.fork_ms += since( f0 );
                                ++st.prefix_forks;
                            }
                            else if ( L > 0 ) ++st.prefix_in_place;
                            const auto p0 = Clock::now();
                            TokenTensor toks( ctx->getDeviceId(), shape_t{ 1, len - L } );
                            Compute::rocmCheck( mila_cdna4_memcpy_h2d( toks.rawData(), prompt.data() + L, static_cast<size_t>( len - L ) * 4, ctx->getStream() ) );
                            net.prefillRow( a.row, toks, len - L, L );      // chunks of the prefill size from L on, as generate() cuts them from its reuse
                            ctx->synchronize();
                            prefix_cache_.extend( a.row, whole.subspan( static_cast<size_t>( L ) ) );
                            st.prefill_ms += since( p0 );
                            ++st.prefills;
                            st.prefill_tokens += len - L;
                            st.reused_tokens[ i ] = L;
                            st.donor_row[ i ] = pl.donor;
                            continue;
                        }
                        if ( a.fork_from < 0 )
                        {
                            const auto p0 = Clock::now();
                            TokenTensor toks( ctx->getDeviceId(), shape_t{ 1, len } );
                            Compute::rocmCheck( mila_cdna4_memcpy_h2d( toks.rawData(), prompt.data(), static_cast<size_t>( len ) * 4, ctx->getStream() ) );
                            net.prefillRow( a.row, toks, len, 0 );
                            ctx->synchronize();
                            st.prefill_ms += since( p0 );
                            filled |= 1u << a.row;
                            ++st.prefills;
                            st.prefill_tokens += len;
                        }
                        else if ( !( ( filled >> a.row ) & 1u ) ) forkFrom( a.fork_from, len );      // (its source: a row of an earlier wave of this round, or filled above)
                        forkFrom( a.row, len );
                    }
                    t0 = Clock::now();
                    for ( const auto& a : wave )
                    {
                        const int b = a.row;
                        const size_t i = static_cast<size_t>( a.request );
                        const auto& prompt = requests[ i ].prompt;
                        position[ static_cast<size_t>( b ) ] = static_cast<dim_t>( prompt.size() );
                        if ( sp[ i ].penalized() ) net.resetTokenTable( b, prompt.data(), prompt.size() );      // before the row's first sample
                        net.sampleRowRequest( b, plan[ i ].greedy ? 0.0f : draw( b ) );      // the first token, from the prefill's logits, then the row's automaton
                        samples[ static_cast<size_t>( b ) ] = 1;
                        if ( logprobs ) { net.enqueueRowLogprobs( b ); lp.readInto( net.tokenLogprobs(), b ); }
                        int32_t token = 0;
                        Compute::rocmCheck( mila_cdna4_memcpy_d2h( &token, net.rowsTokens().data() + b, 4, ctx->getStream() ) );
                        ctx->synchronize();
                        last_token[ static_cast<size_t>( b ) ] = token;
                        net.setRowActive( b, true );
                        (void)deliver( b, token );      // a request that ends here frees its row for the next wave of this round
                    }
                    st.first_sample_ms += since( t0 );
                }
            };
            admitRound();
            std::vector<int32_t> tokens( static_cast<size_t>( R ) );
            while ( queue.live() > 0 )
            {
                const int B = queue.rowsInStep();
                dim_t max_position = 0;
                for ( int b = 0; b < R; ++b ) if ( queue.requestOf( b ) >= 0 ) max_position = std::max( max_position, position[ static_cast<size_t>( b ) ] );
                net.ensureGraphRows( B, max_position, false );      // (the class facts, the row count and the bucket: never a row's parameters)
                for ( int b = 0; b < R; ++b )
                {
                    const int q = queue.requestOf( b );
                    if ( q < 0 ) continue;
                    const RowRequestPlan& pl = plan[ static_cast<size_t>( q ) ];
                    if ( !pl.greedy ) writeRowDraw( b, draw( b ) );      // one draw per live stochastic row, from that request's generator
                    if ( pl.bias.hasRestore() && samples[ static_cast<size_t>( b ) ] == pl.bias.restore_index ) net.commitRowTokenBiasUpdate( b );      // the row's OWN sample index
                }
                net.replayGraphRows();
                queue.step();
                ++st.steps;
                for ( int b = 0; b < R; ++b )
                    if ( queue.requestOf( b ) >= 0 ) { ++position[ static_cast<size_t>( b ) ]; ++samples[ static_cast<size_t>( b ) ]; }
                Compute::rocmCheck( mila_cdna4_memcpy_d2h( tokens.data(), net.rowsTokens().data(), static_cast<size_t>( B ) * 4, ctx->getStream() ) );
                ctx->synchronize();
                if ( logprobs ) lp.read( net.tokenLogprobs(), B );
                for ( int b = 0; b < B; ++b )
                {
                    if ( queue.requestOf( b ) < 0 ) continue;
                    if ( cached )      // the step wrote the KV of the token it was fed -- the sample before this one -- at the row's position
                    {
                        if ( static_cast<dim_t>( prefix_cache_.claim( b ).size() ) + 1 != position[ static_cast<size_t>( b ) ] )
                            throw std::logic_error( "GemmaModel::serveRequests: row " + std::to_string( b ) + "'s claim and position disagree" );
                        prefix_cache_.fed( b, last_token[ static_cast<size_t>( b ) ] );
                    }
                    last_token[ static_cast<size_t>( b ) ] = tokens[ static_cast<size_t>( b ) ];
                    (void)deliver( b, tokens[ static_cast<size_t>( b ) ] );
                }
                admitRound();      // each retired row to the next waiting request, before the next replay
            }
            ctx->synchronize();
            st.captures = static_cast<int64_t>( net.graphRowsCaptureCount() - captures0 );
            if ( stats ) *stats = std::move( st );
            return status;
        }
        template<typename TNet>
        std::vector<GenerateStatus> onGeneratingRequests( TNet& net, std::span<const BatchRequest> requests, const std::function<void( int, int32_t )>& on_token,
                                                          std::vector<std::optional<int32_t>>* final_states )
        {
            Compute::TraceRange tr( "GemmaModel.generateRequests" );
            const int n = static_cast<int>( requests.size() );
            if ( net.maxBatch() < 2 ) throw std::invalid_argument( "GemmaModel::generateRequests: the model was built for one sequence (GemmaModelConfig::withMaxBatch)" );
            if ( n < 1 || n > net.maxBatch() ) throw std::invalid_argument( "GemmaModel::generateRequests: " + std::to_string( n ) + " requests for max_batch " + std::to_string( net.maxBatch() ) );
            std::vector<RowRequestPlan> plan;
            std::vector<typename TNet::SamplingParams> sp;
            for ( int b = 0; b < n; ++b )
            {
                plan.push_back( planRowRequest( requests[ static_cast<size_t>( b ) ], requests[ 0 ].params.logprobs, b, vocabSize(), contextLength(), stopTokens() ) );
                sp.push_back( networkSampling<TNet>( plan.back().sampling ) );
            }
            // ---- nothing was enqueued so far
            kv_token_history_.clear();      // row 0's caches are overwritten: nothing is left to reuse
            last_reuse_ = 0;
            const std::optional<int> logprobs = requests[ 0 ].params.logprobs;
            auto* ctx = net.context();
            const int B = std::max( 2, n );
            net.clearTokenAutomaton();
            for ( int b = 0; b < static_cast<int>( net.maxBatch() ); ++b )
            {
                net.resetRow( b );
                const GenerateParams* p = b < n ? &requests[ static_cast<size_t>( b ) ].params : nullptr;
                // the automaton first: a row with one keeps its bias in the table the automaton composes from
                if ( p && p->automaton ) net.setRowTokenAutomaton( b, *p->automaton ); else net.clearRowTokenAutomaton( b );
                const TokenBiasPlan* bp = b < n ? &plan[ static_cast<size_t>( b ) ].bias : nullptr;
                if ( bp && bp->active )
                {
                    net.setRowTokenBias( b, bp->fill, bp->ids.data(), bp->values.data(), bp->ids.size() );
                    if ( bp->hasRestore() ) net.stageRowTokenBiasUpdate( b, bp->restore_ids.data(), bp->restore_values.data(), bp->restore_ids.size() );
                }
                else net.clearRowTokenBias( b );
            }
            net.setRowsRequests( std::span<const typename TNet::SamplingParams>( sp ), row_draws_dev_ );
            net.setStepLogprobs( logprobs );
            std::vector<std::mt19937_64> rng;
            for ( int b = 0; b < n; ++b ) rng.emplace_back( requests[ static_cast<size_t>( b ) ].seed );
            auto draw = [&]( int b ) { return std::uniform_real_distribution<float>( 0.0f, 1.0f )( rng[ static_cast<size_t>( b ) ] ); };
            TokenLogprobsRows lp;
            lp.top_n = logprobs.value_or( 0 );
            std::vector<dim_t> position( static_cast<size_t>( n ) );
            std::vector<int> emitted( static_cast<size_t>( n ), 0 );
            std::vector<char> active( static_cast<size_t>( n ), 1 );
            std::vector<GenerateStatus> status( static_cast<size_t>( n ), GenerateStatus::Success );
            for ( int b = 0; b < n; ++b )
            {
                const auto& prompt = requests[ static_cast<size_t>( b ) ].prompt;
                const dim_t len = static_cast<dim_t>( prompt.size() );
                TokenTensor toks( ctx->getDeviceId(), shape_t{ 1, len } );
                Compute::rocmCheck( mila_cdna4_memcpy_h2d( toks.rawData(), prompt.data(), static_cast<size_t>( len ) * 4, ctx->getStream() ) );
                net.prefillRow( b, toks, len, 0 );
                ctx->synchronize();
                position[ static_cast<size_t>( b ) ] = len;
                if ( sp[ static_cast<size_t>( b ) ].penalized() ) net.resetTokenTable( b, prompt.data(), prompt.size() );      // before the row's first sample
                net.sampleRowRequest( b, plan[ static_cast<size_t>( b ) ].greedy ? 0.0f : draw( b ) );      // the first token, from the prefill's logits, then the row's automaton
                if ( logprobs ) { net.enqueueRowLogprobs( b ); lp.readInto( net.tokenLogprobs(), b ); }
                net.setRowActive( b, true );
            }
            std::vector<int32_t> tokens( static_cast<size_t>( B ) );
            int live = n;
            bool stepped = false;
            int next_sample = 1;      // the sample index the next rows step produces: the rows step in lockstep, every row's index 0 came behind its prefill
            while ( true )
            {
                Compute::rocmCheck( mila_cdna4_memcpy_d2h( tokens.data(), net.rowsTokens().data(), static_cast<size_t>( B ) * 4, ctx->getStream() ) );
                ctx->synchronize();
                if ( logprobs && stepped ) lp.read( net.tokenLogprobs(), B );      // (a retired row's entries are stale: never reported)
                for ( int b = 0; b < n; ++b )
                {
                    const size_t i = static_cast<size_t>( b );
                    if ( !active[ i ] ) continue;
                    const int32_t token = tokens[ i ];
                    bool retire = true;
                    if ( plan[ i ].stop_ids.contains( token ) ) status[ i ] = GenerateStatus::Success;
                    else
                    {
                        if ( logprobs ) lp.report( requests[ i ].params.on_logprobs, b, b, token );
                        on_token( b, token );
                        ++emitted[ i ];
                        if ( emitted[ i ] >= plan[ i ].max_new ) status[ i ] = GenerateStatus::MaxNewTokensReached;
                        else if ( position[ i ] >= contextLength() ) status[ i ] = GenerateStatus::ContextOverflow;
                        else retire = false;
                    }
                    if ( retire ) { active[ i ] = 0; net.setRowActive( b, false ); --live; }
                }
                if ( live == 0 ) break;
                dim_t max_position = 0;
                for ( int b = 0; b < n; ++b ) if ( active[ static_cast<size_t>( b ) ] ) max_position = std::max( max_position, position[ static_cast<size_t>( b ) ] );
                net.ensureGraphRows( B, max_position, false );      // (the class facts, the row count and the bucket: never a row's parameters)
                for ( int b = 0; b < n; ++b )
                {
                    const size_t i = static_cast<size_t>( b );
                    if ( !active[ i ] ) continue;
                    if ( !plan[ i ].greedy ) writeRowDraw( b, draw( b ) );      // one draw per active stochastic row, from that row's generator
                    if ( plan[ i ].bias.hasRestore() && next_sample == plan[ i ].bias.restore_index ) net.commitRowTokenBiasUpdate( b );      // min_tokens_b: the row's stop tokens are back from this step on
                }
                net.replayGraphRows();
                ++next_sample;
                stepped = true;
                for ( int b = 0; b < n; ++b )
                    if ( active[ static_cast<size_t>( b ) ] ) ++position[ static_cast<size_t>( b ) ];
            }
            ctx->synchronize();
            if ( final_states )
            {
                final_states->assign( static_cast<size_t>( n ), std::nullopt );
                for ( int b = 0; b < n; ++b ) ( *final_states )[ static_cast<size_t>( b ) ] = net.rowTokenAutomatonState( b );
            }
            return status;
        }
        template<typename TNet>
        std::vector<GenerateStatus> onGeneratingBatch( TNet& net, std::span<const std::vector<int32_t>> prompts, const std::function<void( int, int32_t )>& on_token,
                                                       const GenerateParams& params, uint64_t seed )
        {
            Compute::TraceRange tr( "GemmaModel.generateBatch" );
            const int n = static_cast<int>( prompts.size() );
            if ( net.maxBatch() < 2 ) throw std::invalid_argument( "GemmaModel::generateBatch: the model was built for one sequence (GemmaModelConfig::withMaxBatch)" );
            if ( n < 1 || n > net.maxBatch() ) throw std::invalid_argument( "GemmaModel::generateBatch: " + std::to_string( n ) + " prompts for max_batch " + std::to_string( net.maxBatch() ) );
            for ( auto& prompt : prompts )
            {
                if ( prompt.empty() ) throw std::invalid_argument( "GemmaModel::generateBatch: empty prompt" );
                if ( prompt.size() > static_cast<size_t>( contextLength() ) ) throw std::invalid_argument( "GemmaModel::generateBatch: a prompt exceeds the deployment context length" );
                for ( int32_t t : prompt )
                    if ( t < 0 || t >= vocabSize() ) throw std::invalid_argument( "GemmaModel::generateBatch: token id " + std::to_string( t ) + " outside the vocabulary" );
            }
            checkLogprobsRequest( params, vocabSize() );
            std::unordered_set<int32_t> stop_ids;
            if ( params.stop_tokens.empty() ) stop_ids = stopTokens();
            else stop_ids.insert( params.stop_tokens.begin(), params.stop_tokens.end() );
            const bool greedy = isGreedy( params.sampling );
            const typename TNet::SamplingParams sp = networkSampling<TNet>( params.sampling );
            const TokenBiasPlan bias_plan = composeRequestBias( params, stop_ids, vocabSize() );      // (nothing was enqueued yet)
            if ( params.automaton ) throw std::invalid_argument( "GemmaModel::generateBatch: GenerateParams::automaton is not built: one state per row in generateBatch" );
            net.clearTokenAutomaton();
            net.setSamplingFilters( sp );      // the greedy rows samplers' filters: this request's, neutral ones included
            applyRequestBias( net, bias_plan );      // one table for every row, before the first sample
            std::vector<std::mt19937_64> rng;
            for ( int b = 0; b < n; ++b ) rng.emplace_back( seed + static_cast<uint64_t>( b ) );
            auto draw = [&]( int b ) { return std::uniform_real_distribution<float>( 0.0f, 1.0f )( rng[ static_cast<size_t>( b ) ] ); };
            auto sampleRow = [&]( int b ) { if ( greedy ) net.sampleRowGreedy( b ); else net.sampleRowStochastic( b, sp, draw( b ) ); };
            auto* ctx = net.context();
            const int B = std::max( 2, n );      // a rows step carries at least two rows; a row without a prompt stays inactive
            for ( int b = 0; b < static_cast<int>( net.maxBatch() ); ++b ) net.resetRow( b );
            if ( greedy ) net.setRowsSampling( std::nullopt, nullptr );
            else net.setRowsSampling( sp, row_draws_dev_ );      // the rows graph ends in the sampler: token and position bump of every active row
            // log-probabilities: the rows step reports its active rows into the op's device outputs, read back with the tokens; a row's first token is reported alone
            net.setStepLogprobs( params.logprobs );
            TokenLogprobsRows lp;
            lp.top_n = params.logprobs.value_or( 0 );
            std::vector<dim_t> position( static_cast<size_t>( n ) );
            std::vector<int> emitted( static_cast<size_t>( n ), 0 );
            std::vector<char> active( static_cast<size_t>( n ), 1 );
            std::vector<GenerateStatus> status( static_cast<size_t>( n ), GenerateStatus::Success );
            for ( int b = 0; b < n; ++b )
            {
                const auto& prompt = prompts[ static_cast<size_t>( b ) ];
                const dim_t len = static_cast<dim_t>( prompt.size() );
                TokenTensor toks( ctx->getDeviceId(), shape_t{ 1, len } );
                Compute::rocmCheck( mila_cdna4_memcpy_h2d( toks.rawData(), prompt.data(), static_cast<size_t>( len ) * 4, ctx->getStream() ) );
                net.prefillRow( b, toks, len, 0 );
                ctx->synchronize();
                position[ static_cast<size_t>( b ) ] = len;
                if ( sp.penalized() ) net.resetTokenTable( b, prompt.data(), prompt.size() );      // before the row's first sample
                sampleRow( b );      // the first token, from the prefill's logits
                if ( params.logprobs ) { net.enqueueRowLogprobs( b ); lp.readInto( net.tokenLogprobs(), b ); }
                net.setRowActive( b, true );
            }
            const int max_new = params.max_new_tokens.value_or( static_cast<int>( contextLength() ) );
            std::vector<int32_t> tokens( static_cast<size_t>( B ) );
            int live = n;
            bool stepped = false;
            int next_sample = 1;      // the sample index the next rows step produces (every row's index 0 was sampled behind its prefill)
            while ( true )
            {
                Compute::rocmCheck( mila_cdna4_memcpy_d2h( tokens.data(), net.rowsTokens().data(), static_cast<size_t>( B ) * 4, ctx->getStream() ) );
                ctx->synchronize();
                if ( params.logprobs && stepped ) lp.read( net.tokenLogprobs(), B );      // (a retired row's entries are stale: never reported)
                for ( int b = 0; b < n; ++b )
                {
                    const size_t i = static_cast<size_t>( b );
                    if ( !active[ i ] ) continue;
                    const int32_t token = tokens[ i ];
                    bool retire = true;
                    if ( stop_ids.contains( token ) ) status[ i ] = GenerateStatus::Success;
                    else
                    {
                        if ( params.logprobs ) lp.report( params.on_logprobs, b, b, token );
                        on_token( b, token );
                        ++emitted[ i ];
                        if ( emitted[ i ] >= max_new ) status[ i ] = GenerateStatus::MaxNewTokensReached;
                        else if ( position[ i ] >= contextLength() ) status[ i ] = GenerateStatus::ContextOverflow;
                        else retire = false;
                    }
                    if ( retire ) { active[ i ] = 0; net.setRowActive( b, false ); --live; }
                }
                if ( live == 0 ) break;
                dim_t max_position = 0;
                for ( int b = 0; b < n; ++b ) if ( active[ static_cast<size_t>( b ) ] ) max_position = std::max( max_position, position[ static_cast<size_t>( b ) ] );
                net.ensureGraphRows( B, max_position, greedy );      // (re-captures only when the largest active row leaves the captured live-length bucket)
                // stochastic: one draw per active row, from that row's generator in the order the per-row sampler calls took them; the previous replay was drained above
                if ( !greedy )
                    for ( int b = 0; b < n; ++b )
                        if ( active[ static_cast<size_t>( b ) ] ) writeRowDraw( b, draw( b ) );
                if ( bias_plan.hasRestore() && next_sample == bias_plan.restore_index ) net.commitTokenBiasUpdate();      // min_tokens: the stop tokens are back from this step on
                net.replayGraphRows();
                ++next_sample;
                stepped = true;
                for ( int b = 0; b < n; ++b )
                    if ( active[ static_cast<size_t>( b ) ] ) ++position[ static_cast<size_t>( b ) ];
            }
            ctx->synchronize();
            return status;
        }

        GemmaModel( Network net, const GemmaConfig& cfg, const GemmaModelConfig& mc, Serialization::PretrainedMetadata md )
            : network_( std::move( net ) ), network_config_( cfg ), model_config_( mc ), source_metadata_( std::move( md ) )
        {
            const auto dev = std::visit( []( auto& n ) { return n->context()->getDeviceId(); }, network_ );
            // a ring rows model (GemmaConfig::bounded_local_kv_rows): the prefix rule with the rings' geometry (Mila/PrefixCache.h); 0 / 0 otherwise, the flat rule
            std::visit( [&]( auto& n ) { if ( n->rowsRingCapacity() > 0 ) prefix_cache_ = PrefixCache( PrefixCache::kMaxRows, n->config().window, n->rowsRingCapacity() ); }, network_ );
            prompt_dev_ = std::make_unique<TokenTensor>( dev, shape_t{ 1, mc.getPrefillChunk() } );
            decode_token_device_ = std::make_unique<TokenTensor>( dev, shape_t{ 1 } );
            seq_dev_ = std::make_unique<Tensor<TensorDataType::INT32, Compute::RocmDeviceMemoryResource>>( dev, shape_t{ 2 } );      // one 64-bit counter
            auto* ctx = std::visit( []( auto& n ) { return n->context(); }, network_ );
            Compute::rocmCheck( mila_cdna4_memset_zero( seq_dev_->rawData(), 8, ctx->getStream() ) );
            hipCheck( hipHostMalloc( reinterpret_cast<void**>( &ring_host_ ), kSnapshots * sizeof( unsigned long long ), hipHostMallocMapped | hipHostMallocCoherent ), "hipHostMalloc (mapped, coherent token ring)" );      // coherence stated, not left to HIP_HOST_COHERENT: the host polls what the device stores
            std::memset( ring_host_, 0, kSnapshots * sizeof( unsigned long long ) );
            void* dptr = nullptr;
            hipCheck( hipHostGetDevicePointer( &dptr, ring_host_, 0 ), "hipHostGetDevicePointer" );
            ring_dev_ = static_cast<unsigned long long*>( dptr );
            // the uniform draws of the captured stochastic step, the other way round: the host writes slot n % kSnapshots before it launches the replay that takes sample n
            hipCheck( hipHostMalloc( reinterpret_cast<void**>( &draws_host_ ), kSnapshots * sizeof( float ), hipHostMallocMapped | hipHostMallocCoherent ), "hipHostMalloc (mapped, coherent draw ring)" );
            std::memset( draws_host_, 0, kSnapshots * sizeof( float ) );
            hipCheck( hipHostGetDevicePointer( &dptr, draws_host_, 0 ), "hipHostGetDevicePointer" );
            draws_dev_ = static_cast<const float*>( dptr );
            // one draw per row of a rows / chain step with the sampler in it; only a model that has such steps
            if ( cfg.max_batch > 1 || cfg.draft_tokens > 0 )
            {
                hipCheck( hipHostMalloc( reinterpret_cast<void**>( &row_draws_host_ ), kRowDraws * sizeof( float ), hipHostMallocMapped | hipHostMallocCoherent ), "hipHostMalloc (mapped, coherent row draws)" );
                std::memset( row_draws_host_, 0, kRowDraws * sizeof( float ) );
                hipCheck( hipHostGetDevicePointer( &dptr, row_draws_host_, 0 ), "hipHostGetDevicePointer" );
                row_draws_dev_ = static_cast<const float*>( dptr );
            }
            ctx->synchronize();
        }

        /// row b's draw of the next rows / chain step (the step's tail reads it with a system-scope load; no step is in flight when the host writes)
        void writeRowDraw( int b, float r )
        {
            uint32_t bits;
            std::memcpy( &bits, &r, 4 );
            __atomic_store_n( reinterpret_cast<uint32_t*>( row_draws_host_ ) + b, bits, __ATOMIC_RELEASE );
        }
        static bool isGreedy( const SamplingParams& sp ) noexcept { return sp.top_k == 1 || sp.temperature <= 0.0f; }

        // Every sample -- the eager sampler's or the captured step's -- takes the next sequence number on the device and lands in ring slot seq % kSnapshots of
        // host-visible memory.  At most two samples are ever in flight, so a slot is read long before its reuse; the tag makes a stale slot unmistakable.
        unsigned long long* seqCounter() { return reinterpret_cast<unsigned long long*>( seq_dev_->rawData() ); }
        /// sample from the network's current logits into decode_token_device_ (ready for the next decode) and publish it for the host
        template<typename TNet> void enqueueSampleNext( TNet& net, const SamplingParams& sp )
        {
            if ( isGreedy( sp ) ) net.sampleGreedy( *decode_token_device_ );
            else
            {
                net.sampleStochasticRadix( *decode_token_device_, networkSampling<TNet>( sp ), std::uniform_real_distribution<float>( 0.0f, 1.0f )( rng_ ) );
            }
            Compute::rocmCheck( mila_cdna4_snapshot_token( decode_token_device_->data(), seqCounter(), ring_dev_, static_cast<int>( kSnapshots ), net.context()->getStream() ) );
            ++published_;
        }
        /// blocks until sample number `seq` (1-based over this model's lifetime) is host-visible; device work enqueued after it -- the ahead-decoded step --
        /// keeps running.  Polls host memory only; gives up after ~20 s (a wedged device), so a caller never spins forever
        int32_t awaitSampledToken( uint64_t seq )
        {
            volatile unsigned long long* slot = ring_host_ + ( seq % kSnapshots );
            const auto t0 = std::chrono::steady_clock::now();
            for ( uint64_t spins = 0;; ++spins )
            {
                const unsigned long long v = __atomic_load_n( slot, __ATOMIC_ACQUIRE );
                if ( ( v >> 32 ) == ( seq & 0xffffffffull ) ) return static_cast<int32_t>( static_cast<uint32_t>( v ) );
                if ( ( spins & 1023 ) == 1023 )
                {
                    if ( std::chrono::steady_clock::now() - t0 > std::chrono::seconds( 20 ) ) throw std::runtime_error( "GemmaModel::awaitSampledToken: the device did not publish a token within 20 s" );
                    std::this_thread::yield();
                }
            }
        }

        void ensureLogprobRing()
        {
            if ( lp_ring_host_ ) return;
            const size_t bytes = kSnapshots * static_cast<size_t>( Compute::RocmTokenLogprobsOp::recordWords() ) * sizeof( uint32_t );
            hipCheck( hipHostMalloc( reinterpret_cast<void**>( &lp_ring_host_ ), bytes, hipHostMallocMapped | hipHostMallocCoherent ), "hipHostMalloc (mapped, coherent log-probability ring)" );
            std::memset( lp_ring_host_, 0, bytes );
            void* dptr = nullptr;
            hipCheck( hipHostGetDevicePointer( &dptr, lp_ring_host_, 0 ), "hipHostGetDevicePointer" );
            lp_ring_dev_ = static_cast<uint32_t*>( dptr );
        }
        /// awaitSampledToken for the log-probability record of sample `seq` (its tag is stored last): row 0 of `lp` <- the record
        void awaitLogprobRecord( uint64_t seq, int32_t token, TokenLogprobsRows& lp )
        {
            const size_t words = static_cast<size_t>( Compute::RocmTokenLogprobsOp::recordWords() );
            uint32_t* rec = lp_ring_host_ + ( seq % kSnapshots ) * words;
            const auto t0 = std::chrono::steady_clock::now();
            for ( uint64_t spins = 0; __atomic_load_n( rec, __ATOMIC_ACQUIRE ) != static_cast<uint32_t>( seq & 0xffffffffull ); ++spins )
                if ( ( spins & 1023 ) == 1023 )
                {
                    if ( std::chrono::steady_clock::now() - t0 > std::chrono::seconds( 20 ) ) throw std::runtime_error( "GemmaModel::awaitLogprobRecord: the device did not publish a record within 20 s" );
                    std::this_thread::yield();
                }
            if ( static_cast<int32_t>( rec[ 1 ] ) != token || static_cast<int>( rec[ 3 ] ) != lp.top_n ) throw std::runtime_error( "GemmaModel::awaitLogprobRecord: the record is not this sample's" );
            std::memcpy( lp.logprob, rec + 2, 4 );
            std::memcpy( lp.top_ids, rec + 4, static_cast<size_t>( lp.top_n ) * 4 );
            std::memcpy( lp.top_logprobs, rec + 4 + TokenLogprobsRows::kMaxTop, static_cast<size_t>( lp.top_n ) * 4 );
        }

        template<typename TNet>
        ScoreResult onScoring( TNet& net, std::span<const int32_t> tokens, const ScoreParams& params )
        {
            Compute::TraceRange tr( "GemmaModel.score" );
            const dim_t n = static_cast<dim_t>( tokens.size() );
            if ( n < 2 ) throw std::invalid_argument( "GemmaModel::score: at least two tokens (a context and a token to score)" );
            if ( n > contextLength() ) throw std::invalid_argument( "GemmaModel::score: " + std::to_string( n ) + " tokens exceed deployment context length " + std::to_string( contextLength() ) );
            if ( params.first < 1 || params.first > n - 1 ) throw std::invalid_argument( "GemmaModel::score: first " + std::to_string( params.first ) + " outside 1 .. " + std::to_string( n - 1 ) );
            for ( int32_t t : tokens )
                if ( t < 0 || t >= vocabSize() ) throw std::invalid_argument( "GemmaModel::score: token id " + std::to_string( t ) + " outside the vocabulary" );

            dim_t common = 0;
            const dim_t comparable = std::min<dim_t>( n, static_cast<dim_t>( kv_token_history_.size() ) );
            while ( common < comparable && kv_token_history_[ static_cast<size_t>( common ) ] == tokens[ static_cast<size_t>( common ) ] ) ++common;
            dim_t reuse = std::min( common, params.first - 1 );      // position first - 1 is the first one whose head is needed
            if ( reuse > 0 && !net.rewindKvCache( reuse, static_cast<dim_t>( kv_token_history_.size() ) ) ) reuse = 0;
            last_reuse_ = reuse;
            const dim_t chunk = model_config_.getPrefillChunk();
            auto* ctx = net.context();
            if ( !score_targets_dev_ ) score_targets_dev_ = std::make_unique<TokenTensor>( ctx->getDeviceId(), shape_t{ 1, chunk } );
            ScoreResult out;
            const size_t entries = static_cast<size_t>( n - params.first );
            out.logprob.reserve( entries );
            if ( params.argmax ) { out.argmax.reserve( entries ); out.argmax_logprob.reserve( entries ); }
            std::vector<int32_t> targets( static_cast<size_t>( chunk ) );
            kv_token_history_.resize( static_cast<size_t>( reuse ) );
            for ( dim_t p0 = reuse; p0 < n; p0 += chunk )
            {
                const dim_t c = std::min( chunk, n - p0 );
                Compute::rocmCheck( mila_cdna4_memcpy_h2d( prompt_dev_->rawData(), tokens.data() + p0, static_cast<size_t>( c ) * 4, ctx->getStream() ) );
                // positions lo .. hi - 1 of this chunk are scored: position p reports token p + 1
                const dim_t lo = std::max( p0, params.first - 1 ), hi = std::min( p0 + c, n - 1 );
                if ( lo >= hi ) net.prefill( *prompt_dev_, c, p0 );
                else
                {
                    for ( dim_t r = 0; r < c; ++r ) targets[ static_cast<size_t>( r ) ] = p0 + r + 1 < n ? tokens[ static_cast<size_t>( p0 + r + 1 ) ] : -1;
                    Compute::rocmCheck( mila_cdna4_memcpy_h2d( score_targets_dev_->rawData(), targets.data(), static_cast<size_t>( c ) * 4, ctx->getStream() ) );
                    net.prefillScored( *prompt_dev_, c, p0, score_targets_dev_->data(), lo - p0, params.argmax );
                    const size_t at = out.logprob.size(), m = static_cast<size_t>( hi - lo );
                    // rows lo - p0 .. of the chunk were scored; the sequence's last row (no target) is read into the spare slot and dropped
                    const size_t rows = static_cast<size_t>( p0 + c - lo );
                    out.logprob.resize( at + rows );
                    if ( params.argmax ) { out.argmax.resize( at + rows ); out.argmax_logprob.resize( at + rows ); }
                    net.scoreOp().read( static_cast<dim_t>( rows ), out.logprob.data() + at, params.argmax ? out.argmax.data() + at : nullptr,
                                        params.argmax ? out.argmax_logprob.data() + at : nullptr );
                    out.logprob.resize( at + m );
                    if ( params.argmax ) { out.argmax.resize( at + m ); out.argmax_logprob.resize( at + m ); }
                }
                ctx->synchronize();       // prompt_dev_ and the targets are reused by the next chunk
                kv_token_history_.insert( kv_token_history_.end(), tokens.begin() + p0, tokens.begin() + p0 + c );
            }
            for ( float v : out.logprob ) out.sum += static_cast<double>( v );
            return out;
        }

        template<typename TNet>
        GenerateStatus onGenerating( TNet& net, std::span<const int32_t> prompt, const std::function<void( int32_t )>& on_token, const GenerateParams& params, const std::atomic<bool>* stop )
        {
            Compute::TraceRange tr( "GemmaModel.generate" );
            if ( prompt.empty() ) throw std::invalid_argument( "GemmaModel::onGenerating: empty prompt" );
            if ( prompt.size() > static_cast<size_t>( contextLength() ) )
                throw std::invalid_argument( "GemmaModel::onGenerating: prompt length " + std::to_string( prompt.size() ) + " exceeds deployment context length " + std::to_string( contextLength() ) );
            for ( int32_t t : prompt )
                if ( t < 0 || t >= vocabSize() ) throw std::invalid_argument( "GemmaModel::onGenerating: token id " + std::to_string( t ) + " outside the vocabulary" );
            checkLogprobsRequest( params, vocabSize() );
            const typename TNet::SamplingParams net_sampling = networkSampling<TNet>( params.sampling );      // (validates the filters: nothing was enqueued yet)
            std::unordered_set<int32_t> stop_ids;
            if ( params.stop_tokens.empty() ) stop_ids = stopTokens();
            else stop_ids.insert( params.stop_tokens.begin(), params.stop_tokens.end() );
            const TokenBiasPlan bias_plan = composeRequestBias( params, stop_ids, vocabSize() );      // (composed and checked before anything is enqueued)
            checkRequestAutomaton( params, bias_plan, vocabSize() );
            last_automaton_state_.reset();

            // transparent KV prefix reuse: cache positions [0, n) are a function of the first n tokens only, so token equality against what the
            // caches hold is the whole validity test; at least the last prompt position is always prefilled (fresh logits)
            const dim_t seq_len = static_cast<dim_t>( prompt.size() );
            dim_t common = 0;
            const dim_t comparable = std::min<dim_t>( seq_len, static_cast<dim_t>( kv_token_history_.size() ) );
            while ( common < comparable && kv_token_history_[ static_cast<size_t>( common ) ] == prompt[ static_cast<size_t>( common ) ] ) ++common;
            dim_t reuse = std::min( common, seq_len - 1 );
            if ( reuse > 0 && !net.rewindKvCache( reuse, static_cast<dim_t>( kv_token_history_.size() ) ) ) reuse = 0;      // a refused rewind (ring staleness) falls back to the full prefill
            last_reuse_ = reuse;
            const dim_t chunk = model_config_.getPrefillChunk();
            auto* ctx = net.context();
            // the history claims only what the caches hold at every instant: cut to the reused prefix before the first chunk overwrites positions >= reuse,
            // extended chunk by chunk, so a chunk that throws leaves no stale claim for the next generate() to "reuse"
            kv_token_history_.resize( static_cast<size_t>( reuse ) );
            for ( dim_t p0 = reuse; p0 < seq_len; p0 += chunk )
            {
                const dim_t n = std::min( chunk, seq_len - p0 );
                Compute::rocmCheck( mila_cdna4_memcpy_h2d( prompt_dev_->rawData(), prompt.data() + p0, static_cast<size_t>( n ) * 4, ctx->getStream() ) );
                net.prefill( *prompt_dev_, n, p0 );
                ctx->synchronize();       // prompt_dev_ is reused by the next chunk
                kv_token_history_.insert( kv_token_history_.end(), prompt.begin() + p0, prompt.begin() + p0 + n );
            }

            const bool greedy = isGreedy( params.sampling );
            dim_t position = seq_len;
            last_speculation_ = SpeculationStats{};
            // the filters of this request, neutral ones included (the greedy samplers keep no other request's); with a penalty the token table starts from the WHOLE
            // prompt -- a KV-reused prefix, whose chunks were not uploaded above, included -- before the first sample
            net.setSamplingFilters( net_sampling );
            if ( net_sampling.penalized() ) net.resetTokenTable( 0, prompt.data(), prompt.size() );
            applyRequestBias( net, bias_plan );      // the bias table of this request, or none: before the first sample
            // the automaton of this request, or none: uploaded and reset to its start state before the first sample, as the penalties' table is reset above.  The
            // state is followed on the host from the tokens the loop sees (the device word may be one decode-ahead sample further when the request ends)
            if ( params.automaton ) { net.setTokenAutomaton( *params.automaton ); last_automaton_state_ = params.automaton->start; }
            else net.clearTokenAutomaton();
            const bool constrained = bias_plan.active || params.automaton;
            if ( ( greedy || params.speculative_sampling ) && net.draftTokens() > 0 && !net_sampling.filtered() && ( !constrained || params.speculate_constrained ) )
                return onGeneratingSpeculative( net, prompt, on_token, params, stop, stop_ids, greedy, bias_plan );
            // log-probabilities travel like the tokens: every sample's record lands in slot seq % kSnapshots of a second host-visible ring, written by the two launches
            // behind the sampler -- eagerly for the first token, as the captured step's last nodes afterwards
            if ( params.logprobs )
            {
                ensureLogprobRing();
                net.setTokenRing( ring_dev_, static_cast<int>( kSnapshots ), seqCounter() );      // (its sequence counter; the graph setup below repeats the call)
                net.setStepLogprobs( params.logprobs, lp_ring_dev_, static_cast<int>( kSnapshots ) );
            }
            else net.setStepLogprobs( std::nullopt );
            TokenLogprobsRows lp;
            lp.top_n = params.logprobs.value_or( 0 );
            enqueueSampleNext( net, params.sampling );
            if ( params.logprobs ) net.enqueueStepLogprobs( decode_token_device_->data() );
            int emitted = 0;
            const int max_new = params.max_new_tokens.value_or( static_cast<int>( contextLength() ) );
            if ( position < contextLength() )
            {
                // greedy: the captured step ends with the argmax sampler and the publish; stochastic: it ends with the radix sampler, whose last node takes its draw from
                // the draw ring and publishes the same way.  Another kind of request, or other sampling parameters, re-capture (a few ms, once per change)
                net.setSampleInGraph( greedy );
                net.setTokenRing( ring_dev_, static_cast<int>( kSnapshots ), seqCounter() );
                if ( greedy ) net.setGraphSampling( std::nullopt );
                else
                {
                    net.setGraphSampling( net_sampling );
                    net.setDrawRing( draws_dev_, static_cast<int>( kSnapshots ) );
                }
                net.ensureGraph( *decode_token_device_, position );
                net.setDevicePosition( position );
            }
            std::mt19937_64 rng_before_ahead = rng_;
            int next_sample = 1;      // the sample index the next replay produces (index 0 was sampled eagerly above)
            while ( true )
            {
                // (a cancel seen here needs no draw put back: the replay of the previous iteration drew for the sample the eager loop drew at that iteration's end --
                // one draw per sample enqueued, on both loops)
                if ( stop && stop->load( std::memory_order_relaxed ) ) { ctx->synchronize(); return GenerateStatus::ClientCancelled; }
                // decode ahead only when another step could consume its logits: within the token budget and with KV-cache room
                const bool more_steps_allowed = emitted + 1 < max_new;
                const bool cache_has_room = position < contextLength();
                const bool ahead = more_steps_allowed && cache_has_room;
                const uint64_t mine = published_;          // the sample this iteration reports
                if ( ahead )
                {
                    net.ensureGraph( *decode_token_device_, position );      // (re-captures only when the position leaves the captured live-length bucket)
                    if ( !greedy )
                    {
                        // the replay samples the NEXT token before this one is known: one draw per sample, in the order of the eager loop this replaces, and taken
                        // back below when this token ends the request (that loop would not have drawn it: a request leaves the generator where it always did)
                        rng_before_ahead = rng_;
                        const float r = std::uniform_real_distribution<float>( 0.0f, 1.0f )( rng_ );
                        uint32_t bits;
                        std::memcpy( &bits, &r, 4 );
                        __atomic_store_n( reinterpret_cast<uint32_t*>( draws_host_ ) + ( ( published_ + 1 ) % kSnapshots ), bits, __ATOMIC_RELEASE );
                    }
                    // min_tokens: the stop tokens get their values back in stream order immediately before the replay that produces sample index min_tokens
                    if ( bias_plan.hasRestore() && next_sample == bias_plan.restore_index ) net.commitTokenBiasUpdate();
                    net.replayGraph();
                    ++next_sample;
                    ++published_;      // the captured step ends with sampler + publish: the NEXT token
                }
                const int32_t token = awaitSampledToken( mine );
                if ( ahead ) { kv_token_history_.push_back( token ); ++position; }     // the ahead-decode entered it into the caches, whatever it is
                if ( params.automaton ) last_automaton_state_ = params.automaton->step( *last_automaton_state_, token );
                if ( stop_ids.contains( token ) )
                {
                    if ( ahead && !greedy ) rng_ = rng_before_ahead;
                    ctx->synchronize();
                    return GenerateStatus::Success;
                }
                try
                {
                    if ( params.logprobs ) { awaitLogprobRecord( mine, token, lp ); lp.report( params.on_logprobs, 0, 0, token ); }
                    on_token( token );
                }
                catch ( ... )
                {
                    if ( ahead && !greedy ) rng_ = rng_before_ahead;      // the eager loop drew only after on_token returned
                    throw;
                }
                ++emitted;
                if ( !ahead ) return more_steps_allowed ? GenerateStatus::ContextOverflow : GenerateStatus::MaxNewTokensReached;
            }
        }

        /// The decode loop of a withDraftTokens model, entered behind the prefill: greedy, or stochastic with GenerateParams::speculative_sampling.
        /// Each step decodes the current token at `position` together with up to k
        /// drafted successors (padded with token 0 to k: a padded token that happens to verify is a correct token) on the chain step, reads {count, tokens} back and
        /// emits the accepted tokens under generate()'s rules.  It takes the one-row captured step instead when the drafter proposes nothing, when position + k + 1
        /// would pass the context length, or when position and position + k lie in different live-length buckets (the one case where a chain row would not have the
        /// bits it has alone).  Every token is the plain greedy loop's token.  One sync per step, no decode-ahead.
        /// Stochastic: the tail of the chain step samples row t at the draw the plain loop would take for that token (peekDraws) and accepts a draft exactly when it
        /// equals that sample, so every token is the plain stochastic loop's token for the same generator state; only the draws of the tokens that were emitted are
        /// taken (consumeDraws), and the request leaves rng_ where the plain loop leaves it.  The one-row steps are the captured stochastic step of the plain path.
        /// Constrained (GenerateParams::speculate_constrained; bias_plan and the automaton are on the network already): the chain step and the one-row step read the
        /// request's table, the drafts start with the automaton's forced run, and the sample index decides where min_tokens lets a chain step be taken.
        template<typename TNet>
        GenerateStatus onGeneratingSpeculative( TNet& net, std::span<const int32_t> prompt, const std::function<void( int32_t )>& on_token, const GenerateParams& params,
                                                const std::atomic<bool>* stop, const std::unordered_set<int32_t>& stop_ids, bool greedy, const TokenBiasPlan& bias_plan )
        {
            auto* ctx = net.context();
            // A constrained request (speculate_constrained: a bias table and / or an automaton, set on the network by onGenerating).  The host follows the state from
            // the tokens it reads back -- this loop has no decode-ahead, so the device word is never behind it, and is ahead of it only where the request ends inside
            // a chain step's accepted run.  forced[ s ]: the one token state s allows under the request's table (no min_tokens beside an automaton: one table).
            const TokenAutomaton* automaton = params.automaton.get();
            const std::vector<int32_t> forced = automaton ? automaton->forcedTokens( bias_plan ) : std::vector<int32_t>{};
            std::unordered_map<int32_t, float> bias_listed, bias_restored;
            if ( bias_plan.active )
            {
                for ( size_t j = 0; j < bias_plan.ids.size(); ++j ) bias_listed[ bias_plan.ids[ j ] ] = bias_plan.values[ j ];
                for ( size_t j = 0; j < bias_plan.restore_ids.size(); ++j ) bias_restored[ bias_plan.restore_ids[ j ] ] = bias_plan.restore_values[ j ];
            }
            // whether the table lets `t` be sample number `index` of the request (min_tokens: the stop tokens have their values back from restore_index on)
            auto biasFinite = [&]( int32_t t, int index )
            {
                if ( !bias_plan.active ) return true;
                if ( bias_plan.hasRestore() && index >= bias_plan.restore_index )
                    if ( const auto it = bias_restored.find( t ); it != bias_restored.end() ) return std::isfinite( it->second );
                const auto it = bias_listed.find( t );
                return std::isfinite( it != bias_listed.end() ? it->second : bias_plan.fill );
            };
            const int k = static_cast<int>( net.draftTokens() );
            const typename TNet::SamplingParams sp = networkSampling<TNet>( params.sampling );      // (never filtered here: onGenerating sends such requests to the plain loop)
            const int max_new = params.max_new_tokens.value_or( static_cast<int>( contextLength() ) );
            dim_t position = static_cast<dim_t>( prompt.size() );
            std::vector<int32_t> history( prompt.begin(), prompt.end() );
            auto readWords = [&]( int32_t* dst, const int32_t* src, int n )
            {
                Compute::rocmCheck( mila_cdna4_memcpy_d2h( dst, src, static_cast<size_t>( n ) * 4, ctx->getStream() ) );
                ctx->synchronize();
            };
            // log-probabilities: every step of this loop reads its tokens back, and reads the op's device outputs with them (no ring): the one-row step reports row 0,
            // the chain step its accepted rows
            net.setStepLogprobs( params.logprobs );
            TokenLogprobsRows lp;
            lp.top_n = params.logprobs.value_or( 0 );
            // the first token, from the prefill's logits (stochastic: the plain path's call -- one draw, one sequence number)
            if ( greedy ) net.sampleGreedy( *decode_token_device_ );
            else enqueueSampleNext( net, params.sampling );
            if ( params.logprobs ) net.enqueueStepLogprobs( decode_token_device_->data() );
            int32_t token = 0;
            readWords( &token, decode_token_device_->data(), 1 );
            if ( params.logprobs ) lp.read( net.tokenLogprobs(), 1 );
            int emitted = 0;
            // emits one token under generate()'s rules; `at` = the position the token would be decoded at, `b` = its row in lp.  nullopt: go on
            auto emit = [&]( int32_t t, dim_t at, int b = 0 ) -> std::optional<GenerateStatus>
            {
                if ( automaton ) last_automaton_state_ = automaton->step( *last_automaton_state_, t );
                if ( stop_ids.contains( t ) ) return GenerateStatus::Success;
                if ( params.logprobs ) lp.report( params.on_logprobs, 0, b, t );
                on_token( t );
                ++emitted;
                if ( emitted >= max_new ) return GenerateStatus::MaxNewTokensReached;
                if ( at >= contextLength() ) return GenerateStatus::ContextOverflow;
                return std::nullopt;
            };
            if ( auto st = emit( token, position ) ) return *st;
            // the one-row step of this loop: the captured greedy step without the token ring (the loop reads the token back itself), or the plain path's captured
            // stochastic step (its draw slot follows the sequence counter, which comes with the token ring)
            if ( greedy )
            {
                net.setSampleInGraph( true );
                net.setTokenRing( nullptr, 0, nullptr );
                net.setGraphSampling( std::nullopt );
                net.setChainSampling( std::nullopt, nullptr );
            }
            else
            {
                net.setSampleInGraph( false );
                net.setTokenRing( ring_dev_, static_cast<int>( kSnapshots ), seqCounter() );
                net.setGraphSampling( sp );
                net.setDrawRing( draws_dev_, static_cast<int>( kSnapshots ) );
                net.setChainSampling( sp, row_draws_dev_ );
            }
            net.setDevicePosition( position );
            std::vector<int32_t> row( static_cast<size_t>( k ) + 2 );
            while ( true )
            {
                if ( stop && stop->load( std::memory_order_relaxed ) ) { ctx->synchronize(); return GenerateStatus::ClientCancelled; }
                history.push_back( token );
                std::vector<int32_t> drafts;
                int n_forced = 0;
                if ( !automaton && !bias_plan.active )
                {
                    drafts = params.draft ? params.draft( history, k ) : promptLookupDraft( history, k );
                    if ( drafts.size() > static_cast<size_t>( k ) ) drafts.resize( static_cast<size_t>( k ) );
                    for ( int32_t& d : drafts ) if ( d < 0 || d >= vocabSize() ) d = 0;      // a drafter's out-of-range proposal is a wrong draft, not an error
                }
                else
                {
                    // the forced run from the current state, then the drafter on the history extended by it; nothing is drafted behind a stop token, and the
                    // drafter's proposals end at the first one this request can never sample (draft i is sample emitted + i)
                    int q = automaton ? *last_automaton_state_ : 0;
                    bool ended = false;
                    while ( automaton && !ended && static_cast<int>( drafts.size() ) < k && forced[ static_cast<size_t>( q ) ] >= 0 )
                    {
                        const int32_t f = forced[ static_cast<size_t>( q ) ];
                        drafts.push_back( f );
                        q = automaton->step( q, f );
                        ended = stop_ids.contains( f );
                    }
                    n_forced = static_cast<int>( drafts.size() );
                    if ( !ended && n_forced < k )
                    {
                        std::vector<int32_t> extended( history );
                        extended.insert( extended.end(), drafts.begin(), drafts.end() );
                        const std::vector<int32_t> more = params.draft ? params.draft( extended, k - n_forced ) : promptLookupDraft( extended, k - n_forced );
                        for ( int32_t d : more )
                        {
                            if ( ended || static_cast<int>( drafts.size() ) >= k || d < 0 || d >= vocabSize() ) break;
                            if ( ( automaton && !automaton->allows( q, d ) ) || !biasFinite( d, emitted + static_cast<int>( drafts.size() ) ) ) break;
                            drafts.push_back( d );
                            if ( automaton ) q = automaton->step( q, d );
                            ended = stop_ids.contains( d );
                        }
                    }
                }
                // min_tokens: this step's row 0 produces sample `emitted`; the restore goes in front of the step that produces sample restore_index, and a chain step
                // is taken only when its k + 1 samples lie on one side of it (its rows share the ONE table)
                const bool restores = bias_plan.hasRestore();
                if ( restores && emitted == bias_plan.restore_index ) net.commitTokenBiasUpdate();
                const bool one_side = !restores || emitted >= bias_plan.restore_index || emitted + k < bias_plan.restore_index;
                const bool chain = !drafts.empty() && one_side && position + k + 1 <= contextLength() && net.bandBucket( position ) == net.bandBucket( position + k );
                ++last_speculation_.steps;
                if ( !chain )
                {
                    Compute::rocmCheck( mila_cdna4_memcpy_h2d( decode_token_device_->data(), &token, 4, ctx->getStream() ) );
                    net.ensureGraph( *decode_token_device_, position );
                    if ( !greedy )      // the sample's draw, into the slot its sequence number reads
                    {
                        const float r = nextDraw( rng_ );
                        uint32_t bits;
                        std::memcpy( &bits, &r, 4 );
                        __atomic_store_n( reinterpret_cast<uint32_t*>( draws_host_ ) + ( ( published_ + 1 ) % kSnapshots ), bits, __ATOMIC_RELEASE );
                        ++published_;
                    }
                    net.replayGraph();
                    kv_token_history_.push_back( token );
                    ++position;
                    readWords( &token, decode_token_device_->data(), 1 );
                    if ( params.logprobs ) lp.read( net.tokenLogprobs(), 1 );
                    if ( auto st = emit( token, position ) ) return *st;
                    continue;
                }
                const int real = static_cast<int>( drafts.size() ), T = k + 1;
                row[ 0 ] = token;
                for ( int i = 0; i < k; ++i ) row[ static_cast<size_t>( i ) + 1 ] = i < real ? drafts[ static_cast<size_t>( i ) ] : 0;
                net.setChainDrafts( row.data(), T );
                if ( !greedy )      // row t samples at the draw of token emitted + t of the plain loop
                {
                    const std::vector<float> draws = peekDraws( rng_, T );
                    for ( int t = 0; t < T; ++t ) writeRowDraw( t, draws[ static_cast<size_t>( t ) ] );
                }
                net.ensureGraphChain( T, position );
                net.replayGraphChain();
                readWords( row.data(), net.chainResult().data(), T + 1 );
                const int count = row[ 0 ];
                if ( count < 1 || count > T ) throw std::runtime_error( "GemmaModel: the chain step reported " + std::to_string( count ) + " accepted tokens" );
                if ( params.logprobs ) lp.read( net.tokenLogprobs(), count );
                ++last_speculation_.chain_steps;
                last_speculation_.drafted += static_cast<uint64_t>( real );
                last_speculation_.accepted += static_cast<uint64_t>( std::min( count - 1, real ) );
                last_speculation_.forced += static_cast<uint64_t>( n_forced );
                last_speculation_.forced_accepted += static_cast<uint64_t>( std::min( count - 1, n_forced ) );
                // the caches now hold `token` and the count - 1 verified drafts behind it: the accepted tokens but the last, which is the next step's input
                kv_token_history_.push_back( token );
                for ( int i = 0; i + 1 < count; ++i ) kv_token_history_.push_back( row[ static_cast<size_t>( i ) + 1 ] );
                for ( int i = 0; i < count; ++i )
                {
                    token = row[ static_cast<size_t>( i ) + 1 ];
                    if ( i > 0 ) history.push_back( row[ static_cast<size_t>( i ) ] );
                    if ( !greedy ) consumeDraws( rng_, 1 );      // the plain loop sampled this token: its draw is taken; a token behind the request's end never was
                    if ( auto st = emit( token, position + i + 1, i ) ) { ctx->synchronize(); return *st; }
                }
                position += count;
            }
        }

        static constexpr size_t kSnapshots = 8;
        static constexpr size_t kRowDraws = 4;          // rows of a rows / chain step
        SpeculationStats last_speculation_{};
        std::optional<int32_t> last_automaton_state_{};
        Network network_;
        GemmaConfig network_config_;
        GemmaModelConfig model_config_;
        Serialization::PretrainedMetadata source_metadata_;
        std::unique_ptr<TokenTensor> prompt_dev_, decode_token_device_, seq_dev_;
        std::unique_ptr<TokenTensor> score_targets_dev_;      // the targets of a scored chunk, from the first score() on
        std::vector<int32_t> kv_token_history_;
        PrefixCache prefix_cache_;      // what the rows of a max_batch > 1 model hold (serveRequests with ServeParams::prefix_cache)
        dim_t last_reuse_{ 0 };
        std::mt19937_64 rng_{ 0x4d494c41ull };
        unsigned long long* ring_host_{ nullptr };      // pinned + mapped: the device writes, the host polls
        unsigned long long* ring_dev_{ nullptr };       // the same memory through its device address
        float* draws_host_{ nullptr };                  // pinned + mapped: the host writes a draw, the captured stochastic step's last node reads it
        const float* draws_dev_{ nullptr };
        float* row_draws_host_{ nullptr };              // pinned + mapped: one draw per row of a rows / chain step that samples
        const float* row_draws_dev_{ nullptr };
        uint32_t* lp_ring_host_{ nullptr };             // pinned + mapped, from the first request with log-probabilities on: kSnapshots records the device writes, the host polls
        uint32_t* lp_ring_dev_{ nullptr };
        uint64_t published_{ 0 };                       // samples enqueued so far (their sequence numbers are 1 .. published_)
    };
}
