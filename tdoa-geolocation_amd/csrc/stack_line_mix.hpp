// stack_line_mix.hpp -- tdoa_process_sync_drift_locate's middle link (include/tdoa_mi355x.h, "free-running clocks to fix in one
// call"): the clock row of every stack, made on the device from the fine clock lines' clocks and rates
// (stack_sync_drift_fine.hpp), and the pairs' clock differences the delay-table family's kernels take as cdiff
// (stack_locate.hpp).  Which lines, continued to which positions, make which stack's row is data: mix[t] = (a, xa, b, xb, wa, wb),
// and for station s, in 64 bits,
//     cont(l, x)[s] = c16[l][s] + r(16 rate[l][s] x, U D)      row[t][s] = clock_mix_row(cont(a, xa)[s], cont(b, xb)[s], wa, wb)
// r the nearest integer, halves away from zero: tdoa_sync_line_clock16's rule, with x of either sign (a negative x continues a
// line backwards), and stack_clock_mix.hpp's mean.  (l, x, l, x, 1, 0) is line l continued to x.  The kernel knows nothing
// about blocks.
//
// k_line_mix    one workgroup per stack.  The entry is the same for the whole workgroup and is read once.  The stations' rows
//               (S <= 64), one lane each, go to LDS and out as int32 [stack][S]; then the P <= 2016 differences row[j] - row[i],
//               strided over the workgroup in tdoa_locate_set_clock's pair order, go out as long long [stack][P], and beside them
//               U_loc x the differences for the searches on upsampled surfaces.  Plain vector stores.
//
// The host checks the entries (the lines' numbers, |x| <= 65535, 0 <= wa, wb, 1 <= wa + wb <= 65536) and that every continued
// clock fits int32: by the search's bound on |centre|, the gate, the drift and the largest |x|, or word by word where the words
// are the caller's.  The mean is a convex combination of two such clocks, so no value on the device needs a check.  line_cont
// is tdoa_line_mix_rows' and tdoa_sync_line_clock16's too.
#pragma once

#include "stack_clock_mix.hpp"

namespace tdoa {

constexpr int kLineMixThreads = 256;
constexpr int kLineMixMaxX = 65535;

// tdoa_line_mix
struct LineMix {
    int32_t a, xa, b, xb, wa, wb;
};

// a fine line's clock continued to position x, 1/16 sample: clock16 + r(16 rate x, den), den = U D
__host__ __device__ inline long long line_cont(int32_t clock16, int32_t rate, long long x, long long den)
{
    const long long num = (long long)kLocateDelayUnit * rate * x;
    const long long r = (2 * (num < 0 ? -num : num) + den) / (2 * den);
    return (long long)clock16 + (num < 0 ? -r : r);
}

// grid (n_stacks), kLineMixThreads threads.  c16, rate: [line][S], the lines mix names; mix: [stack]; den = U D of the lines;
// S <= kLocateMaxStations, P = S (S - 1) / 2.  rows [stack][S]; cdiff, cdiff_up [stack][P]: row[j] - row[i] and U_loc x it.
__global__ __launch_bounds__(kLineMixThreads) void k_line_mix(const int32_t *c16, const int32_t *rate, const LineMix *mix, int S, int P,
                                                              long long den, int U_loc, int32_t *rows, long long *cdiff, long long *cdiff_up)
{
    __shared__ int32_t row_s[kLocateMaxStations];
    const int t = blockIdx.x, lane = threadIdx.x;
    const LineMix m = mix[t];
    if (lane < S) {
        const size_t ia = (size_t)m.a * S + lane, ib = (size_t)m.b * S + lane;
        const int32_t r = clock_mix_row((int32_t)line_cont(c16[ia], rate[ia], m.xa, den), (int32_t)line_cont(c16[ib], rate[ib], m.xb, den), m.wa, m.wb);
        row_s[lane] = r;
        rows[(size_t)t * S + lane] = r;
    }
    __syncthreads();
    for (int p = lane; p < P; p += kLineMixThreads) {
        int i, j;
        locate_pair(p, S, &i, &j);
        const long long d = (long long)row_s[j] - (long long)row_s[i];
        cdiff[(size_t)t * P + p] = d;
        cdiff_up[(size_t)t * P + p] = d * U_loc;
    }
}

}  // namespace tdoa
