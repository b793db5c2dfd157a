// erm_obs.hpp -- incomplete response patterns (include/ertirt.h: erm_score_masked): the observed mask of a caller's data set turned into every
// subject's COMPACTED CELL LIST, as PURE functions of plain C++.
//
// The mask is obs, uint8 [N][J] column-major as Y is (cell (i, j) at j * N + i): 1 = the cell was administered (its response and its log-time are observed), 0 = it
// was not.  O_i = the observed items of subject i in rising item order, n_i = |O_i|.  The layout is CSR: off [N + 1] (int64, off[0] = 0, off[i + 1] - off[i] = n_i)
// and, for list position k of subject i at off[i] + k, the item index idx (uint16: J <= 896), the response y and the log-time t.  Memory and traffic are
// proportional to the observed cells; the masked tile kernels (erm_marginal_kernels.hpp) run their item sums and their node chains over the list.
//   obs_offsets    counts n_i and leaves the offsets; refuses a mask value above 1.
//   obs_compact    walks the cells once more and fills the lists.  Y and logT at an unobserved cell are NEVER read.  At observed cells a NaN in logT and a
//                  Y above 1 are refused: the NaN wherever it stands (as the complete path refuses a NaN anywhere before a value outside the domain), else the first bad Y.
// Both walk item by item (the caller's arrays are column-major) with a cursor per subject, so a subject's list comes out in rising item order.
// No HIP, no allocation, no environment: the caller owns every array.  g++ compiles this header with -fsanitize=undefined -ftrapv into tests/obs_check
// (tests/test_obs_host.py).
#pragma once
#include <cstdint>

namespace erm {

constexpr int OBS_MAX_ITEMS = 896;        // the item limit of the caller-data entries: an item index fits uint16
enum ObsStatus { OBS_OK = 0, OBS_BAD_MASK = 1, OBS_NAN_LOGT = 2, OBS_BAD_Y = 3 };

// off [N + 1] from the mask.  OBS_BAD_MASK: *bad = the first cell (j * N + i) whose mask value is above 1; off is then unspecified.
inline int obs_offsets(const uint8_t* obs, int64_t N, int J, int64_t* off, int64_t* bad)
{
    for (int64_t i = 0; i <= N; ++i) off[i] = 0;
    for (int j = 0; j < J; ++j) {
        const uint8_t* col = obs + (int64_t)j * N;
        for (int64_t i = 0; i < N; ++i) {
            if (col[i] > 1) { *bad = (int64_t)j * N + i; return OBS_BAD_MASK; }
            off[i + 1] += col[i];
        }
    }
    for (int64_t i = 0; i < N; ++i) off[i + 1] += off[i];
    return OBS_OK;
}

// The lists from the offsets: cur [N] is scratch (the cursors), idx / y [off[N]] and t [off[N]] (logT and t both NULL: a model without response times).
// OBS_NAN_LOGT / OBS_BAD_Y: *bad = the cell; the lists are then unspecified.
inline int obs_compact(const uint8_t* Y, const double* logT, const uint8_t* obs, int64_t N, int J, const int64_t* off, int64_t* cur, uint16_t* idx, uint8_t* y,
                       double* t, int64_t* bad)
{
    for (int64_t i = 0; i < N; ++i) cur[i] = off[i];
    int64_t bad_y = -1;
    for (int j = 0; j < J; ++j) {
        const int64_t c0 = (int64_t)j * N;
        for (int64_t i = 0; i < N; ++i) {
            if (obs[c0 + i] == 0) continue;
            const int64_t k = cur[i]++;
            idx[k] = (uint16_t)j;
            const uint8_t v = Y[c0 + i];
            if (v > 1 && bad_y < 0) bad_y = c0 + i;
            y[k] = v;
            if (logT) {
                const double x = logT[c0 + i];
                if (x != x) { *bad = c0 + i; return OBS_NAN_LOGT; }
                t[k] = x;
            }
        }
    }
    if (bad_y >= 0) { *bad = bad_y; return OBS_BAD_Y; }
    return OBS_OK;
}

}  // namespace erm
