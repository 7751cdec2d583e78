#pragma once
// The scheduling rule of GemmaModel::serveRequests (Mila/GemmaModel.h), host only: no device call, no model, nothing but the standard library -- a CPU program drives it
// (tests/cpp/request_queue.cpp).
//
// A rows model has R rows (2 .. 4) and a queue of n requests (n >= 1, unbounded).  The rule:
//   * requests are admitted in FIFO order, each into the LOWEST free row;
//   * an ADMISSION ROUND is everything between two rows steps (or in front of the first): admit() hands every free row to the next waiting request; the loop runs
//     those admissions, calls retire( row ) for a request that ended at its first sample (a stop token straight after the prefill: zero tokens), and asks admit()
//     again -- the row is free in the same round -- until admit() returns nothing;
//   * among the requests admitted in the SAME ROUND, those with an identical prompt share one prefill: the first is prefilled into its row, a later one forks from the
//     lowest LIVE row that was prefilled or forked with that prompt in this round.  step() ends the round: a row that has stepped is never forked from (its logits are
//     gone, and one re-prefilled position takes another GEMM form), and neither is a row whose request has retired (the loop may hand it on);
//   * after a step's readback the loop calls retire( row ) for every row that ended, then the next round.
// Prompt identity is a class number per request: equal numbers = the same length and the same ids (promptClasses builds them).
// A prefix shorter than a whole prompt, a source row that has stepped or retired, and reuse across rounds and calls are not this rule's: they are the prefix cache
// (Mila/PrefixCache.h), which serveRequests applies, when asked to, to every admission this rule leaves with fork_from < 0.  Row choice and the rule above do not change.
#include <algorithm>
#include <cstdint>
#include <map>
#include <span>
#include <stdexcept>
#include <string>
#include <vector>

namespace Mila::Dnn
{
    /// class numbers of a list of prompts, in order of first appearance: [ i ] == [ j ] exactly when prompt i and prompt j have the same length and the same ids
    inline std::vector<int> promptClasses( const std::vector<std::span<const int32_t>>& prompts )
    {
        struct Less
        {
            bool operator()( std::span<const int32_t> a, std::span<const int32_t> b ) const { return std::lexicographical_compare( a.begin(), a.end(), b.begin(), b.end() ); }
        };
        std::map<std::span<const int32_t>, int, Less> seen;
        std::vector<int> out;
        out.reserve( prompts.size() );
        for ( const auto& p : prompts ) out.push_back( seen.try_emplace( p, static_cast<int>( seen.size() ) ).first->second );
        return out;
    }

    class RequestQueue
    {
    public:
        static constexpr int kMaxRows = 4;
        /// request `request` enters row `row`; fork_from: the row whose prefill it shares, -1 = it prefills for itself
        struct Admission
        {
            int request = -1, row = -1, fork_from = -1;
            bool operator==( const Admission& ) const = default;
        };
        /// where a request ran: its row and the number of rows steps replayed before it was admitted (-1 / -1: not admitted yet)
        struct Placement { int row = -1; int64_t step = -1; };

        RequestQueue( int rows, std::vector<int> prompt_class ) : rows_( rows ), class_( std::move( prompt_class ) ), placement_( class_.size() )
        {
            if ( rows < 2 || rows > kMaxRows ) throw std::invalid_argument( "RequestQueue: " + std::to_string( rows ) + " rows (2 .. 4)" );
            if ( class_.empty() ) throw std::invalid_argument( "RequestQueue: no request" );
            for ( int c : class_ ) if ( c < 0 ) throw std::invalid_argument( "RequestQueue: a negative prompt class" );
            for ( int r = 0; r < kMaxRows; ++r ) { request_[ r ] = -1; fresh_[ r ] = -1; }
        }
        /// one wave of the current round: every free row, lowest first, gets the next waiting request (empty: no free row or nobody waits)
        std::vector<Admission> admit()
        {
            std::vector<Admission> wave;
            for ( int r = 0; r < rows_ && next_ < class_.size(); ++r )
            {
                if ( request_[ r ] >= 0 ) continue;
                const int q = static_cast<int>( next_++ );
                Admission a{ q, r, -1 };
                for ( int s = 0; s < rows_ && a.fork_from < 0; ++s )
                    if ( request_[ s ] >= 0 && fresh_[ s ] == class_[ static_cast<size_t>( q ) ] ) a.fork_from = s;
                request_[ r ] = q;
                fresh_[ r ] = class_[ static_cast<size_t>( q ) ];
                placement_[ static_cast<size_t>( q ) ] = Placement{ r, steps_ };
                ++live_;
                wave.push_back( a );
            }
            return wave;
        }
        /// the request in `row` has ended: the row is free (and no fork source) from now on
        void retire( int row )
        {
            if ( row < 0 || row >= rows_ || request_[ row ] < 0 ) throw std::invalid_argument( "RequestQueue::retire: row " + std::to_string( row ) + " holds no request" );
            request_[ row ] = -1; fresh_[ row ] = -1;
            --live_;
        }
        /// a rows step was replayed: the round is over, no live row holds a bare prefill any more
        void step()
        {
            if ( live_ == 0 ) throw std::logic_error( "RequestQueue::step: no live row" );
            for ( int r = 0; r < rows_; ++r ) fresh_[ r ] = -1;
            ++steps_;
        }
        int rows() const noexcept { return rows_; }
        size_t requests() const noexcept { return class_.size(); }
        size_t waiting() const noexcept { return class_.size() - next_; }
        int live() const noexcept { return live_; }
        bool done() const noexcept { return live_ == 0 && next_ == class_.size(); }
        int64_t steps() const noexcept { return steps_; }
        /// the request in a row, -1 = free
        int requestOf( int row ) const { return request_[ checkedRow( row ) ]; }
        /// the rows a step carries: at least two, up to the highest occupied row
        int rowsInStep() const noexcept
        {
            int hi = 0;
            for ( int r = 0; r < rows_; ++r ) if ( request_[ r ] >= 0 ) hi = r;
            return hi + 1 < 2 ? 2 : hi + 1;
        }
        const Placement& placement( size_t request ) const { return placement_.at( request ); }

    private:
        int checkedRow( int row ) const
        {
            if ( row < 0 || row >= rows_ ) throw std::invalid_argument( "RequestQueue: row " + std::to_string( row ) + " outside the " + std::to_string( rows_ ) + " rows" );
            return row;
        }
        int rows_;
        std::vector<int> class_;
        std::vector<Placement> placement_;
        size_t next_ = 0;
        int live_ = 0;
        int64_t steps_ = 0;
        int request_[ kMaxRows ];      // the request a row holds, -1 = free
        int fresh_[ kMaxRows ];        // the prompt class a LIVE row was prefilled or forked with in this round, -1 = none
    };
}
