// azk_opt_pack.h - how an opt-in reaches its kernels, for the engine files whose kernels take options (azk_begin.hip, azk_moves.hip,
// azk_emit.hip; DESIGN section 18, "One template per kernel family").  Everything is in an unnamed namespace, as the kernels that take the
// packs are: a pack is a kernel's parameter type, and the files' kernels keep the symbols they had in one file.
#pragma once
#include "azk_engine_int.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------
// The opt-ins: playout cap, resignation (19), forced playouts (20), emission under a mask of elements (22), surprise
// weighting (23), Gumbel root (24), random openings (25), move temperature (27), value targets (28).  A kernel an option touches is ONE __global__ template with a bool per option, and
// the options' argument blocks (CapDev, ResignDev, ForcedDev, EmitSym, SurpriseDev, GumbelDev, OpenDev, TempDev, ValueDev) ride on the block in front of them as
// a Pack: that block plus exactly the blocks whose flag is set.  A block that is off is an empty base, which takes no room, so with every
// flag off the Pack IS its first block: the kernel an engine without options launches has the argument layout and the instruction stream it
// always had, and an option costs the others nothing.  The kernels are one line each: the *_body functions behind them take the blocks by
// value, all zero where an option is off (opt), and fold on their flags.  The host turns the engine's state into the template arguments in
// one place per kernel (with_flags, at the end of this file).
// A new option is a flag on each template it touches, an Opt<> in their Packs and a bool at their dispatch.  (An option that combines with few
// of the others can keep the existing kernels' names instead: the Gumbel root's movers are overloads on a pack of their own, GumbelPack.)
// ------------------------------------------------------------------------------------------------
template <class Block, bool ON> struct Opt {};
template <class Block> struct Opt<Block, true> { Block v; };
template <class First, class... Opts> struct Pack : First, Opts... {};
// the option's block out of a pack, or the block of "off" (all zero) where the pack has none
template <class Block, class P> __device__ __forceinline__ Block opt(const P &p) {
    if constexpr (std::is_base_of_v<Opt<Block, true>, P>) return static_cast<const Opt<Block, true> &>(p).v;
    else return Block{};
}
template <class Block> struct Keyed : Block { int key; };        // a block and the move key whose coin this launch flips
template <class First, bool CAP> using CapPack = Pack<First, Opt<CapDev, CAP>>;
template <class First, bool CAP> using CapKeyPack = Pack<First, Opt<Keyed<CapDev>, CAP>>;
template <class First, bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, bool TEMP, bool VALUE>
using MovePack = Pack<First, Opt<CapDev, CAP>, Opt<ResignDev, RESIGN>, Opt<ForcedDev, FORCED>, Opt<SurpriseDev, SURPRISE>, Opt<TempDev, TEMP>, Opt<ValueDev, VALUE>>;
template <bool CAP, bool SYM, bool SURPRISE, bool OPEN, bool VALUE>
using EmitPack = Pack<Dev, Opt<CapDev, CAP>, Opt<EmitSym, SYM>, Opt<SurpriseDev, SURPRISE>, Opt<OpenEmit, OPEN>, Opt<ValueDev, VALUE>>;
// random openings: the kernels that start games take the option's block behind Dev
template <bool OPEN> using OpenPack = Pack<Dev, Opt<OpenDev, OPEN>>;
template <bool CAP, bool OPEN> using RestartPack = Pack<Dev, Opt<CapDev, CAP>, Opt<OpenDev, OPEN>>;
// Gumbel root search combines with resignation only, and the kernels of the other options keep their names: the movers'
// GUMBEL forms are overloads that take this pack
template <class First, bool RESIGN> using GumbelPack = Pack<First, Opt<ResignDev, RESIGN>, Opt<GumbelDev, true>>;
static_assert(sizeof(MovePack<Dev, false, false, false, false, false, false>) == sizeof(Dev) && sizeof(EmitPack<false, false, false, false, false>) == sizeof(Dev) &&
              sizeof(OpenPack<false>) == sizeof(Dev) && sizeof(RestartPack<false, false>) == sizeof(Dev) && sizeof(RestartPack<true, false>) == sizeof(CapPack<Dev, true>) &&
              sizeof(MovePack<ReuseDev, false, false, false, false, false, false>) == sizeof(ReuseDev) &&
              sizeof(MovePack<Dev, true, true, true, false, false, false>) == sizeof(Pack<Dev, Opt<CapDev, true>, Opt<ResignDev, true>, Opt<ForcedDev, true>>) &&
              sizeof(MovePack<Dev, true, true, true, true, false, false>) == sizeof(Pack<Dev, Opt<CapDev, true>, Opt<ResignDev, true>, Opt<ForcedDev, true>, Opt<SurpriseDev, true>>) &&
              sizeof(MovePack<ReuseDev, false, false, false, false, true, false>) == sizeof(Pack<ReuseDev, Opt<TempDev, true>>) &&
              sizeof(MovePack<ReuseDev, false, false, false, false, false, true>) == sizeof(Pack<ReuseDev, Opt<ValueDev, true>>) &&
              sizeof(EmitPack<true, true, false, false, false>) == sizeof(Pack<Dev, Opt<CapDev, true>, Opt<EmitSym, true>>) &&
              sizeof(EmitPack<false, false, false, false, true>) == sizeof(Pack<Dev, Opt<ValueDev, true>>) &&
              sizeof(CapPack<ReuseDev, false>) == sizeof(ReuseDev) && sizeof(CapKeyPack<ReuseDev, false>) == sizeof(ReuseDev), "a pack without options is its first block");

// ---- the host side of the options: runtime flags -> template arguments, engine state -> argument packs ----------------------------------
// f(std::bool_constant per flag), called once: the one place where a kernel's instantiation is chosen
template <class F> void with_flags(F &&f) { f(); }
template <class F, class... Rest> void with_flags(F &&f, bool flag, Rest... rest) {
    if (flag) with_flags([&](auto... more) { f(std::true_type{}, more...); }, rest...);
    else with_flags([&](auto... more) { f(std::false_type{}, more...); }, rest...);
}
// the option's block as a pack takes it: the block where the flag is set, nothing where it is not
template <bool ON, class Block> Opt<Block, ON> on(const Block &b) {
    if constexpr (ON) return {b};
    else return {};
}
template <bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, bool TEMP, bool VALUE, class First>
MovePack<First, CAP, RESIGN, FORCED, SURPRISE, TEMP, VALUE> move_pack(const First &first, const azk_engine *e) {
    return {first, on<CAP>(e->cp), on<RESIGN>(e->rs), on<FORCED>(e->forced()), on<SURPRISE>(e->sp), on<TEMP>(e->tp), on<VALUE>(e->vt)};
}
template <bool CAP, class First> CapKeyPack<First, CAP> cap_key_pack(const First &first, const azk_engine *e, int key) {
    return {first, on<CAP>(Keyed<CapDev>{e->cp, key})};
}

}  // namespace
