// The token automaton of a grammar-constrained request (include/mila_cdna4.h: token automaton).  Host only: no HIP include, so a plain C++ program can test it.
//
// A deterministic automaton over token ids, in the compressed form the device reads: tokens that behave alike in every state share a class,
//   class_of[vocab]   token id -> class (< num_classes)
//   next[S * C]       state x class -> next state (< num_states), or FORBIDDEN: the token may not be emitted in that state
// Stop tokens are ordinary tokens: a state that allows only a stop token ends the request through the stop rule.  validate() checks the limits and the entries;
// checkLive() checks, against the bias table a request composed (Mila/TokenBias.h), that no state reachable from `start` is a dead end -- every reachable state keeps
// a token that the automaton allows AND whose bias is finite, reachability itself counted over such tokens only.  Both run per class: O(vocab + S * C), no device.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "TokenBias.h"

namespace Mila::Dnn
{
    struct TokenAutomaton
    {
        static constexpr uint16_t FORBIDDEN = 0xFFFFu;
        static constexpr int64_t kMaxStates = 65535, kMaxClasses = 65535;
        static constexpr int64_t kMaxNextBytes = int64_t( 256 ) << 20;

        int num_states = 0;                    ///< S
        int num_classes = 0;                   ///< C
        int start = 0;                         ///< the state of a request's first sample
        std::vector<uint16_t> class_of{};      ///< [vocab]
        std::vector<uint16_t> next{};          ///< [S * C]

        int64_t vocab() const noexcept { return static_cast<int64_t>( class_of.size() ); }

        /// throws invalid_argument for what the device entries and the samplers must never see
        void validate( int64_t vocab_size ) const
        {
            const std::string who = "TokenAutomaton";
            if ( num_states < 1 || num_states > kMaxStates ) throw std::invalid_argument( who + ": num_states " + std::to_string( num_states ) + " outside 1 .. 65535" );
            if ( num_classes < 1 || num_classes > kMaxClasses ) throw std::invalid_argument( who + ": num_classes " + std::to_string( num_classes ) + " outside 1 .. 65535" );
            if ( int64_t( num_states ) * num_classes * 2 > kMaxNextBytes ) throw std::invalid_argument( who + ": the transition table exceeds 256 MiB" );
            if ( start < 0 || start >= num_states ) throw std::invalid_argument( who + ": start " + std::to_string( start ) + " is not a state" );
            if ( vocab_size <= 0 || vocab() != vocab_size )
                throw std::invalid_argument( who + ": class_of has " + std::to_string( vocab() ) + " entries, the vocabulary " + std::to_string( vocab_size ) );
            if ( static_cast<int64_t>( next.size() ) != int64_t( num_states ) * num_classes )
                throw std::invalid_argument( who + ": next has " + std::to_string( next.size() ) + " entries, num_states * num_classes is " + std::to_string( int64_t( num_states ) * num_classes ) );
            for ( size_t i = 0; i < class_of.size(); ++i )
                if ( class_of[ i ] >= num_classes ) throw std::invalid_argument( who + ": class_of[" + std::to_string( i ) + "] = " + std::to_string( class_of[ i ] ) + " is not a class" );
            for ( size_t i = 0; i < next.size(); ++i )
                if ( next[ i ] != FORBIDDEN && next[ i ] >= num_states )
                    throw std::invalid_argument( who + ": next[" + std::to_string( i ) + "] = " + std::to_string( next[ i ] ) + " is neither a state nor FORBIDDEN" );
        }

        /// the next state, or the same state for a token the automaton forbids there (what the device step does)
        int step( int state, int32_t token ) const
        {
            const uint16_t n = next[ static_cast<size_t>( state ) * num_classes + class_of[ static_cast<size_t>( token ) ] ];
            return n == FORBIDDEN ? state : n;
        }
        bool allows( int state, int32_t token ) const { return next[ static_cast<size_t>( state ) * num_classes + class_of[ static_cast<size_t>( token ) ] ] != FORBIDDEN; }

        /// forced[s] = the ONE token id that has both a transition and a finite bias in state s, else -1 (no such token, or more than one).  A forced token is known
        /// before the model runs: the masked distribution of state s has one atom, so every sampler returns it.  `bias` as for checkLive (its initial table: a plan
        /// with a restore gives the forced tokens before the restore).  validate() first.  Per class: the count of finite tokens and the sum of their ids, which is
        /// the id where the count is 1.
        std::vector<int32_t> forcedTokens( const TokenBiasPlan& bias ) const
        {
            const size_t C = static_cast<size_t>( num_classes );
            std::vector<int64_t> finite( C, 0 ), id_sum( C, 0 );
            const bool fill_finite = !bias.active || std::isfinite( bias.fill );
            if ( fill_finite )
                for ( size_t i = 0; i < class_of.size(); ++i ) { ++finite[ class_of[ i ] ]; id_sum[ class_of[ i ] ] += static_cast<int64_t>( i ); }
            if ( bias.active )
                for ( size_t j = 0; j < bias.ids.size(); ++j )
                {
                    const uint16_t c = class_of[ static_cast<size_t>( bias.ids[ j ] ) ];
                    const bool f = std::isfinite( bias.values[ j ] );
                    if ( fill_finite && !f ) { --finite[ c ]; id_sum[ c ] -= bias.ids[ j ]; }
                    else if ( !fill_finite && f ) { ++finite[ c ]; id_sum[ c ] += bias.ids[ j ]; }
                }
            std::vector<int32_t> forced( static_cast<size_t>( num_states ), -1 );
            for ( size_t s = 0; s < forced.size(); ++s )
            {
                int64_t count = 0, sum = 0;
                for ( size_t c = 0; c < C && count <= 1; ++c )
                    if ( next[ s * C + c ] != FORBIDDEN && finite[ c ] > 0 ) { count += finite[ c ]; sum += id_sum[ c ]; }
                if ( count == 1 ) forced[ s ] = static_cast<int32_t>( sum );
            }
            return forced;
        }

        /// throws invalid_argument naming the first reachable state (in breadth-first order from start) that keeps no token with a transition and a finite bias;
        /// `bias` is the request's composed table (inactive: every token finite).  validate() first.
        void checkLive( const TokenBiasPlan& bias ) const
        {
            const size_t C = static_cast<size_t>( num_classes );
            // tokens of each class whose bias is finite
            std::vector<int64_t> finite( C, 0 );
            const bool fill_finite = !bias.active || std::isfinite( bias.fill );
            if ( fill_finite )
                for ( uint16_t c : class_of ) ++finite[ c ];
            if ( bias.active )
                for ( size_t j = 0; j < bias.ids.size(); ++j )
                {
                    const uint16_t c = class_of[ static_cast<size_t>( bias.ids[ j ] ) ];
                    const bool f = std::isfinite( bias.values[ j ] );
                    if ( fill_finite && !f ) --finite[ c ];
                    else if ( !fill_finite && f ) ++finite[ c ];
                }
            std::vector<uint8_t> seen( static_cast<size_t>( num_states ), 0 );
            std::vector<int> queue{ start };
            seen[ static_cast<size_t>( start ) ] = 1;
            for ( size_t q = 0; q < queue.size(); ++q )
            {
                const int s = queue[ q ];
                bool live = false;
                for ( size_t c = 0; c < C; ++c )
                {
                    const uint16_t n = next[ static_cast<size_t>( s ) * C + c ];
                    if ( n == FORBIDDEN || finite[ c ] <= 0 ) continue;
                    live = true;
                    if ( !seen[ n ] ) { seen[ n ] = 1; queue.push_back( n ); }
                }
                if ( !live )
                    throw std::invalid_argument( "TokenAutomaton: state " + std::to_string( s ) + " is reachable and a dead end: no token has both a transition and a finite bias there" );
            }
        }
    };
}
