// azk_moves_kld.hip - the kernels of adaptive search budgets (azk_set_kld_stop, azk_set_lead_stop; DESIGN sections 31 and 32) that move games: the asynchronous movers of
// an engine with the option (k_move_async_kld, the k_move_async family once more) and the lock-step checkpoint (k_kld_checkpoint), with the
// calls that launch them.  A file of its own so that the two halves of the mover family compile side by side: azk_moves.o is what the build
// waits for.  The device functions are azk_moves_dev.h's; the arming kernel is azk_begin.hip's.  Built with -ffp-contract=off like every
// engine file.
#include "azk_moves_dev.h"

namespace {

// the asynchronous mover of an engine with adaptive search budgets: k_move_async's family once more (KldPack, azk_moves_dev.h)
template <bool REROOT, bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, bool TEMP, bool VALUE>
__global__ __launch_bounds__(AZK_WAVE) void k_move_async_kld(Dev d, AsyncDev p, KldPack<MovePack<ReuseDev, CAP, RESIGN, FORCED, SURPRISE, TEMP, VALUE>> r) {
    move_async_body<REROOT, CAP, RESIGN, FORCED, SURPRISE, false, TEMP, VALUE, true>(d, p, r, opt<CapDev>(r), opt<ResignDev>(r), opt<ForcedDev>(r), opt<SurpriseDev>(r),
                                                                                     GumbelDev{}, opt<TempDev>(r), opt<ValueDev>(r), r.kd);
}

// the lock-step checkpoint (azk_kld_checkpoint): every game, one wave per game; *released counts the games that got another segment
__global__ __launch_bounds__(AZK_WAVE) void k_kld_checkpoint(Dev d, KldDev kd, int *released) {
    const int g = blockIdx.x;
    if (uniform_i32(d.done[g]) != 0 || uniform_i32(d.sims_done[g]) < uniform_i32(d.budget[0]) || uniform_i32(d.leaf_node[g]) >= 0) return;
    if (kld_judge_one(d, kd, g) && azk_lane() == 0) atomicAdd(released, 1);
}

}  // namespace

void azk_launch_move_async_kld(azk_engine *e, hipStream_t st) {
    const Dev &d = e->d;
    with_flags([&](auto reroot, auto cap, auto resign, auto forced, auto surprise, auto temp, auto value) {
        using P = MovePack<ReuseDev, cap.value, resign.value, forced.value, surprise.value, temp.value, value.value>;
        k_move_async_kld<reroot.value, cap.value, resign.value, forced.value, surprise.value, temp.value, value.value><<<d.G, AZK_WAVE, d.lds_bytes, st>>>(
            d, e->ad, KldPack<P>{move_pack<cap.value, resign.value, forced.value, surprise.value, temp.value, value.value>(e->ru, e), e->kd});
    }, e->ru.mode != 0, e->cp.n_fast != 0, e->rs.v_resign != 0.0, e->forced_k != 0.0, e->sp_on, e->tp_on, e->vt_on);
}

extern "C" {

int32_t azk_kld_checkpoint(azk_engine *e, int32_t *released_host, void *stream) {
    if (!e || !released_host) return AZK_ERR_ARG;
    if (!adaptive_on(e)) { e->err = "azk_kld_checkpoint: no adaptive search budget is set (azk_set_kld_stop / azk_set_lead_stop)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_kld_checkpoint: the asynchronous movers judge their games themselves"; return AZK_ERR_STATE; }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(e, hipMemsetAsync(e->n_leaf_scratch, 0, sizeof(int), st));
    k_kld_checkpoint<<<e->d.G, AZK_WAVE, 0, st>>>(e->d, e->kd, e->n_leaf_scratch);
    HIPCHK(e, hipMemcpyAsync(released_host, e->n_leaf_scratch, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return AZK_OK;
}

}  // extern "C"
