// azk_tail_common.h - what the two forms of the cls-row tail's GEMM links share (azk_nn.hip k_tail_gemm: whole K in registers;
// azk_tail.hip k_tail_lds: LDS-staged wide links): the argument block and the epilogue selectors; the epilogue arithmetic (gelu_erf) is
// azk_nn_common.h's, so that a link computes the same values whichever kernel runs it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace azk_tail {

struct TailArgs {
    const unsigned short *A; int lda, a_batch;
    const uint4 *Wp; long long w_batch;          // uint4 elements between batches
    int M, N, nbatch;                            // N = output columns per batch (multiple of 64 * NWC)
    const int *count;
    const float *bias;                           // [nbatch * N] or null
    unsigned short *out; int ldo;
    const unsigned short *resid; int ldr;
    float ln_eps;
    const float *stats_in; int stats_groups;     // LayerNorm of A: [M][stats_groups][2] partial (sum, sum of squares) of every A row, written by the producer
    float *stats_out;                            // optional: this GEMM's own partials [M][nbatch * N / 64][2] of the bf16-rounded output rows
    float *logits, *values; int action_dim;
    int wave_slots;                              // k_tail_gemm: waves of the launched instantiation the device holds at once (set by launch_tail)
    const float *csum;                           // k_tail_lds, LayerNorm in the epilogue: [N] column sums of the (bf16) weight
};

enum { TAIL_EPI_BF16 = 0, TAIL_EPI_GELU = 1, TAIL_EPI_RESID = 2, TAIL_EPI_HEADS = 3 };

}  // namespace azk_tail
