// erm_farm_diag.hpp -- the chunk arithmetic of the chain farm's joint convergence diagnostics (erm_farm_get_diagnostics and its three siblings), as
// PURE functions.  The farm gathers the post-burn-in rows of a chunk of columns of every chain into ONE interleaved scratch [row = m L + l][nc] on chain 0's
// device and runs the estimator kernels on it; the chunk length follows from a fixed scratch budget.  A trace is up to N J ~ 1e8 columns wide, so every count here
// is an int64 and the byte counts are computed without overflow:
//     farm_diag_bytes       bytes of the gathered draws of nc columns: nc * Tn * L * elem, saturated at INT64_MAX
//     farm_diag_chunk_len   columns per chunk: the most whose gathered draws fit `budget` bytes (one column if not even one fits), no more than `cap` (cap <= 0: no
//                           cap) and than the block is wide; where more chunks follow, a chunk of four columns or more is a multiple of four, so that every
//                           chunk starts on a 16-byte boundary of a float or double row (farm_gather_kernel's wide accesses); a block that fits one chunk is not split
//     FarmDiagChunks        the chunk list of a block of ncol columns: count() chunks, chunk i = columns [at(i).c0, at(i).c0 + at(i).nc) -- they cover every column
//                           exactly once, in order, and none but the last is shorter than the chunk length
// The same header is compiled by g++ with -fsanitize=undefined into tests/farm_diag_check (tests/test_farm_diag_host.py).  No HIP, no allocation, no environment.
#pragma once
#include <cstdint>

namespace erm {

constexpr int64_t FARM_DIAG_BUDGET = (int64_t)256 << 20;      // bytes of gathered draws per chunk (rank_diag_run stages as much again for the rank kernels)
constexpr int64_t FARM_DIAG_I64_MAX = 0x7fffffffffffffffll;

// a * b for non-negative a, b, saturated
inline int64_t farm_diag_mul_sat(int64_t a, int64_t b) { return (a == 0 || b == 0) ? 0 : (a > FARM_DIAG_I64_MAX / b ? FARM_DIAG_I64_MAX : a * b); }
inline int64_t farm_diag_bytes(int64_t nc, int64_t Tn, int64_t L, int64_t elem) { return farm_diag_mul_sat(farm_diag_mul_sat(nc, Tn), farm_diag_mul_sat(L, elem)); }

inline int64_t farm_diag_chunk_len(int64_t ncol, int64_t Tn, int64_t L, int64_t elem, int64_t budget, int64_t cap)
{
    const int64_t per_col = farm_diag_bytes(1, Tn, L, elem);
    int64_t chunk = per_col > 0 ? budget / per_col : ncol;
    if (cap > 0 && chunk > cap) chunk = cap;
    if (chunk > ncol) chunk = ncol;
    if (chunk >= 4 && chunk < ncol) chunk &= ~(int64_t)3;      // (one chunk that holds the whole block starts at column 0 and is followed by none: left as it is)
    return chunk < 1 ? 1 : chunk;
}

struct FarmDiagChunk { int64_t c0, nc; };
struct FarmDiagChunks {
    int64_t ncol, chunk;
    int64_t count() const { return ncol <= 0 ? 0 : (ncol - 1) / chunk + 1; }
    FarmDiagChunk at(int64_t i) const { const int64_t c0 = i * chunk; return { c0, ncol - c0 < chunk ? ncol - c0 : chunk }; }      // i < count(): i * chunk < ncol
};
inline FarmDiagChunks farm_diag_chunks(int64_t ncol, int64_t Tn, int64_t L, int64_t elem, int64_t budget, int64_t cap)
{
    return { ncol, farm_diag_chunk_len(ncol, Tn, L, elem, budget, cap) };
}

}  // namespace erm
