// azk_sym_map.h - the D4 elements of a board, shared by the three places that turn one: evaluation under a symmetry (azk_sym.hip), (state,
// pi, z) emission under a mask of elements (azk_emit.hip) and the replay batch gather (azk_replay.hip).  include/azk.h
// (azk_set_eval_symmetry) has the numbering and src_s.  Not part of the ABI.
#pragma once
#include <stdint.h>

#include "azk_device.h"

namespace azk_eng {

// source cell (row-major) of output cell (i, c) under element s of the emission's order (d4_source in azk_emit.hip), select-based: an
// element is "transpose?" then "flip the source row?" and "flip the source column?".  Elements that transpose exist on square boards only.
__device__ __forceinline__ int sym_source_rc(int s, int i, int c, int R, int C) {
    const bool t = (0xB8u >> s) & 1u, fi = (0xD4u >> s) & 1u, fj = (0x5Au >> s) & 1u;
    int si = t ? c : i, sj = t ? i : c;
    si = fi ? R - 1 - si : si;
    sj = fj ? C - 1 - sj : sj;
    return si * C + sj;
}

// the same for output cell j = i * C + c, split by multiplication: inv_cols = ceil(65536 / C) is exact for j < 65536 / C only - the engine's
// boards (make_game: at most 400 cells and 30 columns); inv_cols = 0 puts every j in row 0 (a board of one row, whatever its width)
__device__ __forceinline__ int sym_source(int s, int j, int R, int C, unsigned inv_cols) {
    const int i = (int)(((unsigned)j * inv_cols) >> 16);
    return sym_source_rc(s, i, j - i * C, R, C);
}

// the elements a geometry admits, as a bit mask (bit s = element s): all eight on a square board with one action per cell, {0, 1, 2, 6}
// with one action per cell and rows != cols, {0, 1} with one action per column (Connect4: gravity keeps the rows), else the identity alone
inline uint32_t sym_valid_mask(int rows, int cols, int action_dim) {
    if (action_dim == rows * cols) return rows == cols ? 0xFFu : 0x47u;
    return action_dim == cols ? 0x03u : 0x01u;
}

// a mask's elements in ascending order, four bits each, lowest first (SymDev.valid, EmitSym.els); *n = how many
inline uint32_t sym_pack(uint32_t mask, int *n) {
    uint32_t packed = 0;
    int k = 0;
    for (int s = 0; s < 8; s++)
        if ((mask >> s) & 1u) packed |= (uint32_t)s << (4 * k++);
    *n = k;
    return packed;
}

// what is wrong with a caller's mask of elements for this geometry (nullptr: nothing): it needs the identity, no bit above 7 and only
// elements sym_valid_mask admits
inline const char *sym_mask_error(uint32_t mask, int rows, int cols, int action_dim) {
    if (mask & ~0xFFu) return "the element mask has bits above 7";
    if (!(mask & 1u)) return "the element mask needs bit 0 (the identity)";
    if (mask & ~sym_valid_mask(rows, cols, action_dim)) return "the board's geometry does not admit an element of the mask";
    return nullptr;
}

}  // namespace azk_eng
