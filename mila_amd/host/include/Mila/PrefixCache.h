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
// RINGS.  PrefixCache( rows, window, capacity ) with window > 0 is the rule of a model whose sliding-window layers sit on rings of `capacity` cells, position p at cell
// p % capacity (GemmaConfig::bounded_local_kv_rows), and whose forks copy a ring layer's live band [max( 0, len - window ), len) only.  A claim then says less than "all of
// [0, |H_r|)": on the ring layers only the positions from a VALID-FROM bound on are intact.  Beside H_r each row keeps
//   high_r        the furthest length ever written since the row was last written from position 0 (a cut claim keeps it: the stale tail is still in the ring), and
//   from_r        the lowest position a band fork is known to have left intact in the row (0 when the row was prefilled from 0);
//   valid_from_r  = max( 0, from_r, high_r - capacity + 1 ): the writes up to high_r have reused the cells of every position below high_r - capacity, and the cell of
//                   position high_r - capacity is the one the next write takes.  It counts as taken: a rows step also writes a row that is in the step but not live --
//                   the K / V of a stale token at the row's position word, |H_r| <= high_r.
// A continuation from `reuse` reads down to reuse - window + 1:
//   usable( s, reuse ) = max( 0, reuse - window + 1 ) >= valid_from_s.
// For reuse >= window that is reuse - window >= max( len_fork - window, high_s - capacity ) -- the ring rule of RocmGqaOp::rewindKvCache, high - reuse <= capacity - window,
// and a forked row's bound max( 0, len - window ).  Below the window it is stricter than that form read with max( 0, . ): a row written up to exactly `capacity`, or forked
// at exactly `window`, may have lost position 0, which a shorter prefix would read.
// The bound is a LOWER bound, so a shorter prefix of the same row is never usable where a longer one is not: plan() counts an unusable row's match as 0 and nothing else
// changes -- reuse = min( max over usable s of m_s, len - 1 ), where usable is asked at min( m_s, len - 1 ).
//   adopt( r, tokens )     AFTER a band fork into row r: H_r = tokens, high_r = |tokens|, from_r = max( 0, |tokens| - window + 1 ) (the fork copies one position more,
//                          |tokens| - window; the donor was not asked for it);
//   beginWrite( r, 0 )     the row is about to be written from position 0: high_r = from_r = 0;   beginWrite( r, keep > 0 ) keeps both;
//   extend / fed           raise high_r to |H_r|.
// With window = capacity = 0 (the default) no bound exists and every answer is the one above.
//
// Not here: copying more than the live band to keep a forked row's donation range, choosing the free row by best match, any eviction beyond "a written row loses its
// claim", sharing with generate()'s row-0 history.
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

        explicit PrefixCache( int rows = kMaxRows, int64_t window = 0, int64_t capacity = 0 ) : rows_( rows ), window_( window ), capacity_( capacity )
        {
            if ( rows < 1 || rows > kMaxRows ) throw std::invalid_argument( "PrefixCache: " + std::to_string( rows ) + " rows (1 .. 4)" );
            if ( window < 0 || capacity < 0 || ( window > 0 ) != ( capacity > 0 ) || capacity < window )
                throw std::invalid_argument( "PrefixCache: window " + std::to_string( window ) + " and ring capacity " + std::to_string( capacity ) + " (both 0, or 0 < window <= capacity)" );
        }
        Plan plan( int row, std::span<const int32_t> prompt, int64_t min_prefix = 1 ) const
        {
            checkedRow( row );
            if ( prompt.empty() ) throw std::invalid_argument( "PrefixCache::plan: empty prompt" );
            if ( min_prefix < 1 ) throw std::invalid_argument( "PrefixCache::plan: min_prefix " + std::to_string( min_prefix ) + " (>= 1)" );
            int64_t m[ kMaxRows ] = {}, best = 0;
            const int64_t last = static_cast<int64_t>( prompt.size() ) - 1;
            for ( int s = 0; s < rows_; ++s )
            {
                m[ s ] = common( claim_[ s ], prompt );
                if ( !usable( s, std::min( m[ s ], last ) ) ) m[ s ] = 0;      // (a shorter prefix of the same row is no better: the bound is a lower bound)
                best = std::max( best, m[ s ] );
            }
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
            if ( keep == 0 ) high_[ row ] = from_[ row ] = 0;      // written from position 0: whatever the ring held no longer counts
        }
        void extend( int row, std::span<const int32_t> tokens ) { auto& h = claim_[ checkedRow( row ) ]; h.insert( h.end(), tokens.begin(), tokens.end() ); wrote( row ); }
        void fed( int row, int32_t token ) { claim_[ checkedRow( row ) ].push_back( token ); wrote( row ); }
        /// after a band fork of `tokens` into the row: on the ring layers only [max( 0, len - window ), len) is there
        void adopt( int row, std::span<const int32_t> tokens )
        {
            claim_[ checkedRow( row ) ].assign( tokens.begin(), tokens.end() );
            high_[ row ] = static_cast<int64_t>( tokens.size() );
            from_[ row ] = window_ > 0 ? std::max<int64_t>( 0, high_[ row ] - window_ + 1 ) : 0;
        }
        void invalidate( int row ) { claim_[ checkedRow( row ) ].clear(); }
        void clear() noexcept { for ( auto& h : claim_ ) h.clear(); }
        int rows() const noexcept { return rows_; }
        int64_t window() const noexcept { return window_; }
        int64_t capacity() const noexcept { return capacity_; }
        int64_t high( int row ) const { return high_[ checkedRow( row ) ]; }
        /// the lowest position of row `row` whose ring contents are intact (0 without rings)
        int64_t validFrom( int row ) const { checkedRow( row ); return window_ > 0 ? std::max<int64_t>( { 0, from_[ row ], high_[ row ] - capacity_ + 1 } ) : 0; }
        /// may a continuation from `reuse` run on what row `row` holds (given that its claim matches that far)?
        bool usable( int row, int64_t reuse ) const { return window_ <= 0 || std::max<int64_t>( 0, reuse - window_ + 1 ) >= validFrom( row ); }
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
        void wrote( int row ) { high_[ row ] = std::max( high_[ row ], static_cast<int64_t>( claim_[ row ].size() ) ); }
        int rows_;
        int64_t window_, capacity_;
        int64_t high_[ kMaxRows ] = {}, from_[ kMaxRows ] = {};
        std::vector<int32_t> claim_[ kMaxRows ];
    };
}
