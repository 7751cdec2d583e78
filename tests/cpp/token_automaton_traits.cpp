// Host-only facts of the token automaton (compiled AND run, without a GPU, by tests/test_token_automaton_cpu.py with the host flags of mila_amd/build.py):
// GenerateParams::automaton and the transformer's automaton surface exist, TokenAutomaton::validate refuses what the device must never see, checkLive names a dead end
// -- one of the automaton's own, and one that exists only because of a ban -- and checkRequestAutomaton refuses min_tokens beside an automaton.
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>

#include "Mila/GemmaModel.h"

using namespace Mila::Dnn;

static_assert( std::is_same_v<decltype( GenerateParams::automaton ), std::shared_ptr<const TokenAutomaton>> );

template<typename Net>
concept AutomatonSurface = requires( Net& n, const TokenAutomaton& a )
{
    n.setTokenAutomaton( a );
    n.resetTokenAutomaton();
    n.clearTokenAutomaton();
    { n.tokenAutomatonOn() } -> std::same_as<bool>;
    { n.tokenAutomatonState() } -> std::same_as<int32_t>;
};
static_assert( AutomatonSurface<GemmaTransformer<Quant::Weight::NoWeightQuant>> && AutomatonSurface<GemmaTransformer<Quant::Weight::PerChannelFp8<>>> &&
               AutomatonSurface<GemmaTransformer<Quant::Weight::PerGroupFp4<128>>> );

template<typename M>
concept ModelSurface = requires( const M& m ) { { m.lastAutomatonState() } -> std::same_as<std::optional<int32_t>>; };
static_assert( ModelSurface<GemmaModel<DeviceType::Rocm, TensorDataType::BF16>> );

template<typename F> static std::string invalidMessage( F&& f )
{
    try { f(); }
    catch ( const std::invalid_argument& e ) { return e.what(); }
    return "";
}

int main()
{
    int bad = 0;
    auto expect = [&]( bool ok, const char* what ) { if ( !ok ) { std::printf( "FAILED: %s\n", what ); ++bad; } };
    constexpr uint16_t F = TokenAutomaton::FORBIDDEN;
    constexpr int64_t V = 8;
    // two classes: tokens 0 .. 5 (class 0) and 6, 7 (class 1).  state 0 -0-> 0, -1-> 1; state 1 -1-> 2; state 2 -0-> 2
    TokenAutomaton a;
    a.num_states = 3; a.num_classes = 2; a.start = 0;
    a.class_of = { 0, 0, 0, 0, 0, 0, 1, 1 };
    a.next = { 0, 1, F, 2, 2, F };
    expect( invalidMessage( [&] { a.validate( V ); } ).empty(), "a valid automaton validates" );
    expect( a.step( 0, 6 ) == 1 && a.step( 1, 0 ) == 1 && a.step( 1, 7 ) == 2 && a.allows( 0, 3 ) && !a.allows( 1, 3 ), "step and allows" );
    { auto b = a; b.start = 3; expect( !invalidMessage( [&] { b.validate( V ); } ).empty(), "start >= S throws" ); }
    { auto b = a; b.class_of[ 2 ] = 2; expect( !invalidMessage( [&] { b.validate( V ); } ).empty(), "a class_of entry >= C throws" ); }
    { auto b = a; b.next[ 1 ] = 3; expect( !invalidMessage( [&] { b.validate( V ); } ).empty(), "a next entry that is neither a state nor FORBIDDEN throws" ); }
    { auto b = a; b.num_states = 0; expect( !invalidMessage( [&] { b.validate( V ); } ).empty(), "S = 0 throws" ); }
    { auto b = a; b.num_classes = 65536; expect( !invalidMessage( [&] { b.validate( V ); } ).empty(), "C = 65536 throws" ); }
    { auto b = a; b.num_states = 65535; b.num_classes = 4096; expect( !invalidMessage( [&] { b.validate( V ); } ).empty(), "S * C * 2 above 256 MiB throws" ); }
    expect( !invalidMessage( [&] { a.validate( V + 1 ); } ).empty(), "another vocabulary throws" );
    { auto b = a; b.next.pop_back(); expect( !invalidMessage( [&] { b.validate( V ); } ).empty(), "a short next table throws" ); }

    TokenBiasPlan none;
    expect( invalidMessage( [&] { a.checkLive( none ); } ).empty(), "no dead end without a bias" );
    // a dead end of the automaton's own: state 2 allows nothing
    { auto b = a; b.next[ 4 ] = F; expect( invalidMessage( [&] { b.checkLive( none ); } ).find( "state 2" ) != std::string::npos, "the automaton's own dead end names state 2" ); }
    // a dead end that exists only because of a ban: state 1 allows class 1 = tokens 6 and 7
    TokenBiasRequest rq;
    rq.banned_tokens = { 6 };
    expect( invalidMessage( [&] { a.checkLive( composeTokenBias( rq, V ) ); } ).empty(), "one of the two tokens banned: state 1 lives" );
    rq.banned_tokens = { 6, 7 };
    // ... but now class 1 is gone everywhere, so state 1 is no longer reachable: no dead end, and state 0 lives through class 0
    expect( invalidMessage( [&] { a.checkLive( composeTokenBias( rq, V ) ); } ).empty(), "reachability runs over doubly-allowed tokens only" );
    { auto b = a; b.next[ 0 ] = F; expect( invalidMessage( [&] { b.checkLive( composeTokenBias( rq, V ) ); } ).find( "state 0" ) != std::string::npos, "the ban makes state 0 a dead end" ); }
    rq.banned_tokens = { 0, 1, 2, 3, 4, 5 };
    expect( invalidMessage( [&] { a.checkLive( composeTokenBias( rq, V ) ); } ).find( "state 2" ) != std::string::npos, "class 0 banned: state 2, reachable through class 1, is the dead end" );
    rq = TokenBiasRequest{};
    rq.allowed_tokens = { 1, 6 };
    expect( invalidMessage( [&] { a.checkLive( composeTokenBias( rq, V ) ); } ).empty(), "an allow-list that keeps one token of each class" );
    rq.allowed_tokens = { 6 };
    expect( invalidMessage( [&] { a.checkLive( composeTokenBias( rq, V ) ); } ).find( "state 2" ) != std::string::npos, "an allow-list without class 0: state 2 is the dead end" );

    GenerateParams gp;
    gp.automaton = std::make_shared<const TokenAutomaton>( a );
    expect( invalidMessage( [&] { checkRequestAutomaton( gp, none, V ); } ).empty(), "a request with a valid automaton" );
    gp.min_tokens = 1;
    expect( invalidMessage( [&] { checkRequestAutomaton( gp, none, V ); } ).find( "min_tokens" ) != std::string::npos, "min_tokens beside an automaton throws" );
    gp.automaton.reset();
    expect( invalidMessage( [&] { checkRequestAutomaton( gp, none, V ); } ).empty(), "min_tokens alone is not this check's business" );
    if ( !bad ) std::printf( "token automaton traits OK\n" );
    return bad;
}
