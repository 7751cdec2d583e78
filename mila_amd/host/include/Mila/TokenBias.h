// Request-to-table composition of the logit-bias controls (include/mila_cdna4.h: logit bias).  Host only: no HIP include, so a plain C++ program can test it.
//
// Four request controls are ONE device mechanism, a dense table of `vocab` fp32 values (finite or -inf) that the samplers add to the capped logit:
//   logit_bias       id -> finite value, added to the token's logit
//   banned_tokens    ids that must never be sampled                      (-inf)
//   allowed_tokens   a closed answer set: every other id is forbidden     (fill -inf, the allowed ids get their bias or 0)
//   min_tokens       no stop token before the n-th sampled token          (the stop ids are -inf until sample index min_tokens is due)
// A ban wins over an allow.  composeTokenBias() turns them into the initial table (one fill value and an (id, value) list), the restore list (the stop ids with the
// values they have in the table WITHOUT min_tokens) and the sample index at which the restore is due, and refuses what cannot be served.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <map>
#include <optional>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace Mila::Dnn
{
    struct TokenBiasRequest
    {
        std::vector<std::pair<int32_t, float>> logit_bias{};      ///< id -> finite additive bias; an id at most once
        std::vector<int32_t> banned_tokens{};                     ///< never sampled
        std::vector<int32_t> allowed_tokens{};                    ///< non-empty: only these may be sampled
        std::vector<int32_t> stop_tokens{};                       ///< the request's stop set (read only while min_tokens > 0)
        int min_tokens = 0;                                       ///< no stop token among the first min_tokens samples
        std::optional<int> max_new_tokens{};                      ///< where set, min_tokens may not exceed it
        bool any() const noexcept { return !logit_bias.empty() || !banned_tokens.empty() || !allowed_tokens.empty() || min_tokens != 0; }
    };

    struct TokenBiasPlan
    {
        bool active = false;                      ///< the request needs a bias table at all (false: every list below is empty)
        float fill = 0.0f;                        ///< the value of every id not listed: 0, or -inf under an allow-list
        std::vector<int32_t> ids{};               ///< ascending, unique
        std::vector<float> values{};              ///< values[j] is the table value of ids[j]
        std::vector<int32_t> restore_ids{};       ///< the stop ids (ascending, unique); empty unless min_tokens > 0
        std::vector<float> restore_values{};      ///< ... with their values of the table without min_tokens
        int restore_index = 0;                    ///< the restore goes in front of the step that produces this sample index (the first sampled token is index 0)
        bool hasRestore() const noexcept { return !restore_ids.empty(); }
    };

    inline TokenBiasPlan composeTokenBias( const TokenBiasRequest& rq, int64_t vocab )
    {
        constexpr float kNegInf = -std::numeric_limits<float>::infinity();
        const char* who = "composeTokenBias";
        if ( vocab <= 0 ) throw std::invalid_argument( std::string( who ) + ": vocab must be positive" );
        auto checkId = [&]( int32_t id, const char* what )
        {
            if ( id < 0 || id >= vocab ) throw std::invalid_argument( std::string( who ) + ": " + what + " id " + std::to_string( id ) + " outside the vocabulary" );
        };
        if ( rq.min_tokens < 0 ) throw std::invalid_argument( std::string( who ) + ": min_tokens must not be negative" );
        if ( rq.max_new_tokens && rq.min_tokens > *rq.max_new_tokens ) throw std::invalid_argument( std::string( who ) + ": min_tokens exceeds max_new_tokens" );
        std::map<int32_t, float> bias;
        for ( const auto& [id, v] : rq.logit_bias )
        {
            checkId( id, "logit_bias" );
            if ( !std::isfinite( v ) ) throw std::invalid_argument( std::string( who ) + ": the logit_bias of id " + std::to_string( id ) + " is not finite" );
            if ( !bias.emplace( id, v ).second ) throw std::invalid_argument( std::string( who ) + ": id " + std::to_string( id ) + " occurs twice in logit_bias" );
        }
        for ( int32_t id : rq.banned_tokens ) checkId( id, "banned" );
        for ( int32_t id : rq.allowed_tokens ) checkId( id, "allowed" );
        const bool hold_stops = rq.min_tokens > 0 && !rq.stop_tokens.empty();
        if ( hold_stops )
            for ( int32_t id : rq.stop_tokens ) checkId( id, "stop" );

        TokenBiasPlan plan;
        plan.active = !rq.logit_bias.empty() || !rq.banned_tokens.empty() || !rq.allowed_tokens.empty() || hold_stops;
        if ( !plan.active ) return plan;

        // the table without min_tokens
        std::map<int32_t, float> table;
        if ( !rq.allowed_tokens.empty() )
        {
            plan.fill = kNegInf;
            for ( int32_t id : rq.allowed_tokens )
            {
                const auto it = bias.find( id );
                table[ id ] = it != bias.end() ? it->second : 0.0f;
            }
        }
        else table = bias;
        for ( int32_t id : rq.banned_tokens ) table[ id ] = kNegInf;      // a ban wins over an allow
        auto finiteCount = [&]( const std::map<int32_t, float>& t )
        {
            int64_t listed_finite = 0;
            for ( const auto& kv : t ) listed_finite += std::isfinite( kv.second ) ? 1 : 0;
            return plan.fill == 0.0f ? ( vocab - static_cast<int64_t>( t.size() ) ) + listed_finite : listed_finite;
        };
        if ( finiteCount( table ) <= 0 ) throw std::invalid_argument( std::string( who ) + ": no token is left with a finite bias" );

        std::map<int32_t, float> initial = table;
        if ( hold_stops )
        {
            const std::set<int32_t> stops( rq.stop_tokens.begin(), rq.stop_tokens.end() );
            for ( int32_t id : stops )
            {
                const auto it = table.find( id );
                plan.restore_ids.push_back( id );
                plan.restore_values.push_back( it != table.end() ? it->second : plan.fill );
                initial[ id ] = kNegInf;
            }
            plan.restore_index = rq.min_tokens;
            if ( finiteCount( initial ) <= 0 ) throw std::invalid_argument( std::string( who ) + ": min_tokens leaves no token with a finite bias before the restore" );
        }
        for ( const auto& [id, v] : initial )
        {
            if ( v == plan.fill ) continue;      // (what the fill already says)
            plan.ids.push_back( id );
            plan.values.push_back( v );
        }
        return plan;
    }
}
