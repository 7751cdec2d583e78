// Host-only facts of speculative sampling (compiled AND run, without a GPU, by tests/test_sample_radix_rows_cpu.py with the host flags of mila_amd/build.py): the draw
// bookkeeping of the speculative loop -- peekDraws( T ) followed by consumeDraws( n ) leaves the generator where n plain draws leave it, and the peeked values are the
// plain draws -- and the default of GenerateParams::speculative_sampling.
#include <cstdio>
#include <random>

#include "Mila/GemmaModel.h"

using namespace Mila::Dnn;

int main()
{
    int bad = 0;
    auto expect = [&]( bool ok, const char* what ) { if ( !ok ) { std::printf( "FAILED: %s\n", what ); ++bad; } };
    expect( GenerateParams{}.speculative_sampling == false, "speculative_sampling is off by default" );
    for ( uint64_t seed : { 0ull, 7ull, 0x4d494c41ull } )
        for ( int T = 2; T <= 4; ++T )
            for ( int n = 1; n <= T; ++n )
            {
                std::mt19937_64 plain( seed ), mine( seed );
                (void)nextDraw( plain ); (void)nextDraw( mine );      // somewhere inside a request
                const std::mt19937_64 before = mine;
                const std::vector<float> peeked = peekDraws( mine, T );
                expect( mine == before, "peekDraws leaves the generator where it was" );
                expect( static_cast<int>( peeked.size() ) == T, "peekDraws gives T draws" );
                std::mt19937_64 walk = plain;
                for ( int t = 0; t < T; ++t )
                {
                    const float r = std::uniform_real_distribution<float>( 0.0f, 1.0f )( walk );
                    expect( peeked[ static_cast<size_t>( t ) ] == r, "the peeked draws are the plain loop's next draws, in order" );
                    expect( r >= 0.0f && r <= 1.0f, "a draw lies in [0, 1]" );
                }
                consumeDraws( mine, n );
                for ( int i = 0; i < n; ++i ) (void)std::uniform_real_distribution<float>( 0.0f, 1.0f )( plain );
                expect( mine == plain, "peek( T ) then consume( n ) leaves the generator where n plain draws leave it" );
                expect( nextDraw( mine ) == nextDraw( plain ), "and the following draw is the same" );
            }
    std::mt19937_64 a( 3 ), b( 3 );
    consumeDraws( a, 0 );
    expect( a == b && peekDraws( a, 0 ).empty(), "nothing peeked, nothing consumed" );
    if ( !bad ) std::printf( "spec sampling draws OK\n" );
    return bad;
}
