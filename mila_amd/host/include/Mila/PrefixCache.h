#pragma once
// The prefix-reuse rule of GemmaModel::serveRequests( ..., ServeParams{ prefix_cache } ) (Mila/GemmaModel.h), host only: no device call, no model, nothing but the
// standard library -- a CPU program drives it against a shadow cache (tests/cpp/prefix_cache.cpp).
//
// A rows model keeps every row on unbounded caches: position p of a sequence sits at cache index p of its row, in every layer, and the KV of positions [0, n) depends on
// the first n tokens only.  So what a row holds can be named by a token vector.  Row r has a CLAIM H_r: "cache positions [0, |H_r|) of row r, in every layer, hold the KV
// of exactly these tokens".  A claim outlives the request that wrote it: a retired row keeps its claim until the row is written.
//
//   plan( r, prompt, min_prefix ) -> { donor, reuse }
//     m_s   = the length of the common prefix of H_s and the prompt, for EVERY row s -- live, free, or r itself;
//     reuse = min( max_s m_s, len - 1 ): the last prompt position is always prefilled, so the logits are fresh (generate()'s rule);
//     reuse < min_prefix (or reuse == 0) -> { -1, 0 }: a whole prefill;
//     donor = r itself when m_r reaches reuse (in place: no copy), otherwise the lowest row whose m_s does.
//   beginWrite( r, keep )  cuts H_r to `keep` BEFORE anything writes the row at positions >= keep;
//   extend( r, tokens )    AFTER a fork or a prefill chunk has completed: those positions now hold these tokens;
//   fed( r, token )        AFTER a rows step, for the token that step was fed into row r (the token sampled one step earlier; never the last sample of a request);
//   invalidate( r ), clear().
// A claim never says more than the caches hold at that instant.  An admission that throws between beginWrite and extend leaves the cut claim: nothing stale.
//
// ORDER INSIDE A ROUND.  The admissions of a round are planned and executed one after the other, in the queue's order (FIFO, lowest free row; Mila/RequestQueue.h):
// admission k sees the claims as the admissions before it left them -- their fresh whole prompts included, and the claims they cut excluded.  Planning a whole wave up
// front would let two admissions name each other's row as the donor after the first has already overwritten it.
//
// Not here: copying only a windowed layer's live band (a claim would need a valid-from bound), choosing the free row by best match, any eviction beyond "a written row
// loses its claim", sharing with generate()'s row-0 history.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <span>
#include <stdexcept>
#include <string>
#include <vector>

namespace Mila::Dnn
{
    class PrefixCache
    {
    public:
        static constexpr int kMaxRows = 4;
        /// donor: the row whose positions [0, reuse) the request takes over (-1: none, the request's own row: in place); reuse: how many
        struct Plan
        {
            int donor = -1;
            int64_t reuse = 0;
            bool operator==( const Plan& ) const = default;
        };

        explicit PrefixCache( int rows = kMaxRows ) : rows_( rows )
        {
            if ( rows < 1 || rows > kMaxRows ) throw std::invalid_argument( "PrefixCache: " + std::to_string( rows ) + " rows (1 .. 4)" );
        }
        Plan plan( int row, std::span<const int32_t> prompt, int64_t min_prefix = 1 ) const
        {
            checkedRow( row );
            if ( prompt.empty() ) throw std::invalid_argument( "PrefixCache::plan: empty prompt" );
            if ( min_prefix < 1 ) throw std::invalid_argument( "PrefixCache::plan: min_prefix " + std::to_string( min_prefix ) + " (>= 1)" );
            int64_t m[ kMaxRows ] = {}, best = 0;
            for ( int s = 0; s < rows_; ++s ) { m[ s ] = common( claim_[ s ], prompt ); best = std::max( best, m[ s ] ); }
            const int64_t reuse = std::min<int64_t>( best, static_cast<int64_t>( prompt.size() ) - 1 );
            if ( reuse < min_prefix ) return {};
            if ( m[ row ] >= reuse ) return { row, reuse };
            for ( int s = 0; s < rows_; ++s ) if ( m[ s ] >= reuse ) return { s, reuse };
            return {};      // (unreachable: best >= reuse)
        }
        void beginWrite( int row, size_t keep )
        {
            auto& h = claim_[ checkedRow( row ) ];
            if ( keep > h.size() ) throw std::logic_error( "PrefixCache::beginWrite: row " + std::to_string( row ) + " keeps " + std::to_string( keep ) + " of " + std::to_string( h.size() ) + " claimed positions" );
            h.resize( keep );
        }
        void extend( int row, std::span<const int32_t> tokens ) { auto& h = claim_[ checkedRow( row ) ]; h.insert( h.end(), tokens.begin(), tokens.end() ); }
        void fed( int row, int32_t token ) { claim_[ checkedRow( row ) ].push_back( token ); }
        void invalidate( int row ) { claim_[ checkedRow( row ) ].clear(); }
        void clear() noexcept { for ( auto& h : claim_ ) h.clear(); }
        int rows() const noexcept { return rows_; }
        const std::vector<int32_t>& claim( int row ) const { return claim_[ checkedRow( row ) ]; }

    private:
        static int64_t common( const std::vector<int32_t>& h, std::span<const int32_t> p )
        {
            const size_t n = std::min( h.size(), p.size() );
            size_t i = 0;
            while ( i < n && h[ i ] == p[ i ] ) ++i;
            return static_cast<int64_t>( i );
        }
        int checkedRow( int row ) const
        {
            if ( row < 0 || row >= rows_ ) throw std::invalid_argument( "PrefixCache: row " + std::to_string( row ) + " outside the " + std::to_string( rows_ ) + " rows" );
            return row;
        }
        int rows_;
        std::vector<int32_t> claim_[ kMaxRows ];
    };
}
