// The scheduling rule of GemmaModel::serveRequests, alone (compiled with the host compiler and -fsanitize=address,undefined and RUN by tests/test_request_queue_cpu.py;
// host code only: this file includes nothing but Mila/RequestQueue.h).  A request is a (prompt class, length) pair: length = the tokens it emits, 0 = it ends at its
// first sample.  drive() is the loop of serveRequests without a device: rounds of admit() until nothing comes, one step, the retirements of that step.
#include <cstdio>
#include <numeric>
#include <stdexcept>
#include <vector>

#include "Mila/RequestQueue.h"

using namespace Mila::Dnn;
using Admission = RequestQueue::Admission;

static int failures = 0;
#define CHECK( cond ) do { if ( !( cond ) ) { std::printf( "FAILED line %d: %s\n", __LINE__, #cond ); ++failures; } } while ( 0 )

struct Run
{
    std::vector<Admission> admissions;          // in the order they were made
    std::vector<int64_t> admitted_at;           // per admission: steps replayed before it
    std::vector<int> finish_order;              // requests in the order they ended
    std::vector<int> rows_in_step;              // per step
    int64_t steps = 0;
    int prefills = 0, forks = 0;
};

static Run drive( int R, const std::vector<int>& cls, const std::vector<int>& length )
{
    RequestQueue q( R, cls );
    Run run;
    std::vector<int> left( static_cast<size_t>( R ), 0 );
    auto round = [&]
    {
        for ( auto wave = q.admit(); !wave.empty(); wave = q.admit() )
        {
            int last_row = -1;
            for ( const auto& a : wave )
            {
                CHECK( a.row > last_row );      // lowest free row first
                last_row = a.row;
                CHECK( q.requestOf( a.row ) == a.request );
                if ( a.fork_from >= 0 )
                {
                    // the source is another LIVE row, holding the same prompt, admitted in this round
                    CHECK( a.fork_from != a.row && q.requestOf( a.fork_from ) >= 0 );
                    const int src = q.requestOf( a.fork_from );
                    CHECK( src >= 0 && cls[ static_cast<size_t>( src ) ] == cls[ static_cast<size_t>( a.request ) ] );
                    CHECK( src >= 0 && q.placement( static_cast<size_t>( src ) ).step == q.steps() );
                    ++run.forks;
                }
                else ++run.prefills;
                run.admissions.push_back( a );
                run.admitted_at.push_back( q.steps() );
                CHECK( q.placement( static_cast<size_t>( a.request ) ).row == a.row && q.placement( static_cast<size_t>( a.request ) ).step == q.steps() );
            }
            for ( const auto& a : wave )      // the first sample: a request of length 0 ends here, a request of length 1 at its first token
            {
                left[ static_cast<size_t>( a.row ) ] = length[ static_cast<size_t>( a.request ) ] - 1;
                if ( left[ static_cast<size_t>( a.row ) ] <= 0 ) { run.finish_order.push_back( a.request ); q.retire( a.row ); }
            }
        }
    };
    round();
    while ( q.live() > 0 )
    {
        run.rows_in_step.push_back( q.rowsInStep() );
        q.step();
        for ( int b = 0; b < R; ++b )
        {
            if ( q.requestOf( b ) < 0 ) continue;
            if ( --left[ static_cast<size_t>( b ) ] <= 0 ) { run.finish_order.push_back( q.requestOf( b ) ); q.retire( b ); }
        }
        round();
    }
    CHECK( q.done() && q.waiting() == 0 );
    run.steps = q.steps();
    return run;
}

static std::vector<int> distinct( size_t n ) { std::vector<int> c( n ); std::iota( c.begin(), c.end(), 0 ); return c; }

int main()
{
    {   // FIFO, lowest free row: R = 3, lengths 3 5 2 4 1: the first three start together; row 2 frees first (after 1 step), then row 0
        const Run r = drive( 3, distinct( 5 ), { 3, 5, 2, 4, 1 } );
        const std::vector<Admission> want{ { 0, 0, -1 }, { 1, 1, -1 }, { 2, 2, -1 }, { 3, 2, -1 }, { 4, 0, -1 } };
        CHECK( r.admissions == want );
        CHECK( ( r.admitted_at == std::vector<int64_t>{ 0, 0, 0, 1, 2 } ) );
        // request 4 (one token) ends in its admission round, after step 2; request 3 runs steps 2 .. 4, request 1 steps 1 .. 4
        CHECK( r.steps == 4 && r.prefills == 5 && r.forks == 0 );
        CHECK( ( r.finish_order == std::vector<int>{ 2, 0, 4, 1, 3 } ) );
        CHECK( ( r.rows_in_step == std::vector<int>{ 3, 3, 3, 3 } ) );
    }
    {   // zero-token requests free their row in the same round: R = 2, requests 0 and 2 end at their first sample
        const Run r = drive( 2, distinct( 5 ), { 0, 3, 0, 0, 2 } );
        const std::vector<Admission> want{ { 0, 0, -1 }, { 1, 1, -1 }, { 2, 0, -1 }, { 3, 0, -1 }, { 4, 0, -1 } };
        CHECK( r.admissions == want );
        CHECK( ( r.admitted_at == std::vector<int64_t>{ 0, 0, 0, 0, 0 } ) );      // all five before the first step
        CHECK( r.steps == 2 );      // request 1: 3 tokens = first sample + 2 steps
        CHECK( ( r.finish_order == std::vector<int>{ 0, 2, 3, 4, 1 } ) );
    }
    {   // identical prompts in one round: one prefill plus forks, whatever lies between them
        const Run r = drive( 4, { 0, 1, 0, 0, 2 }, { 4, 4, 4, 4, 4 } );
        const std::vector<Admission> head{ { 0, 0, -1 }, { 1, 1, -1 }, { 2, 2, 0 }, { 3, 3, 0 } };
        CHECK( r.admissions.size() == 5 && std::vector<Admission>( r.admissions.begin(), r.admissions.begin() + 4 ) == head );
        CHECK( r.prefills == 3 && r.forks == 2 );
        CHECK( r.admissions[ 4 ].fork_from == -1 && r.admitted_at[ 4 ] == 3 );
    }
    {   // identical prompts in different rounds do not fork: the same prompt at queue positions 0 and 5 on two rows, and everywhere on two rows with a step between
        const Run r = drive( 2, { 0, 1, 2, 3, 4, 0 }, { 2, 2, 2, 2, 2, 2 } );
        CHECK( r.prefills == 6 && r.forks == 0 );
        const Run same = drive( 2, { 0, 0, 0, 0 }, { 3, 2, 3, 3 } );
        // round 0: request 0 prefills, request 1 forks; after step 1 request 1 ends and request 2 enters row 1 beside a row that has stepped: it prefills
        const std::vector<Admission> want{ { 0, 0, -1 }, { 1, 1, 0 }, { 2, 1, -1 }, { 3, 0, -1 } };
        CHECK( same.admissions == want && same.prefills == 3 && same.forks == 1 );
    }
    {   // a fork source must be LIVE: request 0 ends at its first sample, request 2 takes its row in the same round and forks from nobody -- request 1 (another
        // prompt) is the only live row; request 3, the same prompt as 2, arrives in a later round
        const Run r = drive( 2, { 0, 1, 0, 0 }, { 0, 3, 2, 2 } );
        const std::vector<Admission> want{ { 0, 0, -1 }, { 1, 1, -1 }, { 2, 0, -1 }, { 3, 0, -1 } };
        CHECK( r.admissions == want && r.forks == 0 );
        // ... while a live row of an EARLIER WAVE of the same round is a source: 0 ends at once, 1 lives, 2 (the prompt of 1) enters row 0 and forks from row 1
        const Run w = drive( 2, { 0, 1, 1 }, { 0, 3, 3 } );
        const std::vector<Admission> want_w{ { 0, 0, -1 }, { 1, 1, -1 }, { 2, 0, 1 } };
        CHECK( w.admissions == want_w && w.forks == 1 && w.prefills == 2 );
    }
    {   // n < R and n = 1: a step carries two rows at least
        const Run two = drive( 4, distinct( 2 ), { 3, 2 } );
        CHECK( two.steps == 2 && ( two.rows_in_step == std::vector<int>{ 2, 2 } ) );
        const Run one = drive( 3, distinct( 1 ), { 4 } );
        CHECK( one.steps == 3 && ( one.rows_in_step == std::vector<int>{ 2, 2, 2 } ) && one.admissions.size() == 1 && one.admissions[ 0 ] == ( Admission{ 0, 0, -1 } ) );
        const Run none = drive( 2, distinct( 1 ), { 0 } );
        CHECK( none.steps == 0 && none.finish_order.size() == 1 );
        // the highest occupied row decides: rows 0 and 1 retire, row 2 lives on
        const Run high = drive( 3, distinct( 3 ), { 2, 2, 5 } );
        CHECK( ( high.rows_in_step == std::vector<int>{ 3, 3, 3, 3 } ) );
    }
    {   // 50 requests on R = 2: every request once, FIFO, and the step count of the greedy two-row schedule computed by hand below
        std::vector<int> len( 50 ), cls( 50 );
        for ( int i = 0; i < 50; ++i ) { len[ static_cast<size_t>( i ) ] = ( i * 7 ) % 5; cls[ static_cast<size_t>( i ) ] = i % 3; }      // lengths 0 .. 4, three prompts
        const Run r = drive( 2, cls, len );
        CHECK( r.admissions.size() == 50 && r.finish_order.size() == 50 );
        for ( size_t i = 0; i < r.admissions.size(); ++i ) CHECK( r.admissions[ i ].request == static_cast<int>( i ) );
        std::vector<int> seen( 50, 0 );
        for ( int q : r.finish_order ) ++seen[ static_cast<size_t>( q ) ];
        for ( int s : seen ) CHECK( s == 1 );
        // an independent model of two rows: each row is busy until a step number.  At step `now` the free rows, lowest first, take the next requests (one wave);
        // a request of length 0 or 1 takes no step -- its first token comes with the admission -- and leaves its row free for the next wave at the same `now`
        int64_t busy[ 2 ] = { 0, 0 }, now = 0;
        for ( int i = 0; i < 50; )
        {
            now = std::max( now, std::min( busy[ 0 ], busy[ 1 ] ) );
            const bool free_row[ 2 ] = { busy[ 0 ] <= now, busy[ 1 ] <= now };
            for ( int b = 0; b < 2 && i < 50; ++b )
            {
                if ( !free_row[ b ] ) continue;
                CHECK( r.admissions[ static_cast<size_t>( i ) ].row == b && r.admitted_at[ static_cast<size_t>( i ) ] == now );
                busy[ b ] = now + std::max( 0, len[ static_cast<size_t>( i ) ] - 1 );
                ++i;
            }
        }
        CHECK( r.steps == std::max( busy[ 0 ], busy[ 1 ] ) );
        CHECK( r.steps < std::accumulate( len.begin(), len.end(), 0 ) );
    }
    {   // what the queue refuses
        auto throws = []( auto&& f ) { try { f(); } catch ( const std::exception& ) { return true; } return false; };
        CHECK( throws( [] { RequestQueue q( 1, { 0 } ); } ) && throws( [] { RequestQueue q( 5, { 0 } ); } ) && throws( [] { RequestQueue q( 2, {} ); } ) );
        CHECK( throws( [] { RequestQueue q( 2, { 0, -1 } ); } ) );
        RequestQueue q( 2, { 0, 0, 0 } );
        CHECK( throws( [&] { q.step(); } ) && throws( [&] { q.retire( 0 ); } ) );
        CHECK( q.admit().size() == 2 && q.admit().empty() && q.waiting() == 1 && q.live() == 2 );
        CHECK( throws( [&] { q.retire( 2 ); } ) && throws( [&] { (void)q.requestOf( -1 ); } ) );
        // prompt classes: the same ids = the same class, a prefix is another prompt
        const std::vector<std::vector<int32_t>> p{ { 1, 2, 3 }, { 1, 2 }, { 1, 2, 3 }, {}, { 3, 2, 1 }, { 1, 2 } };
        std::vector<std::span<const int32_t>> spans( p.begin(), p.end() );
        CHECK( ( promptClasses( spans ) == std::vector<int>{ 0, 1, 0, 2, 3, 1 } ) );
    }
    if ( failures ) { std::printf( "%d checks failed\n", failures ); return 1; }
    std::printf( "request queue OK\n" );
    return 0;
}
