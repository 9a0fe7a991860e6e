// stack_line_mix.hpp -- the middle link of the two calls that go from reference blocks to a fix (include/tdoa_mi355x.h, "clocks
// to fix in one call" and "free-running clocks to fix in one call"): the clock row of every stack, made on the device from the
// clocks a fine clock stage left there (stack_sync_fine.hpp's clocks; stack_sync_drift_fine.hpp's clocks and rates), and the
// pairs' clock differences the delay-table family's kernels take as cdiff (stack_locate.hpp).  Which sources, continued to which
// positions, make which stack's row is data: mix[t] = (a, xa, b, xb, wa, wb), and for station s, in 64 bits,
//     cont(l, x)[s] = c16[l][s] + r(16 rate[l][s] x, U D)      T = wa cont(a, xa)[s] + wb cont(b, xb)[s]
//     row[t][s] = sgn(T) ((2 |T| + den) div (2 den)),  den = wa + wb
// r and the row the nearest integer, halves away from zero: tdoa_sync_line_clock16's rule, with x of either sign (a negative x
// continues a line backwards), then the weighted mean.  The sum is rounded, not an increment: on exact halves of opposite sign
// this differs from a ramp that rounds its steps.  (l, x, l, x, 1, 0) is line l continued to x; (a, 0, b, 0, 1, 1) is the
// midpoint rule (|T| + 1) div 2.  Without rates (rate == nullptr) the sources are clocks that stand still, cont(l, x) = c16[l]:
// a clock mix (a, b, wa, wb) is the entry (a, 0, b, 0, wa, wb), widened on the host.  The kernel knows nothing about blocks.
//
// k_line_mix    one workgroup per stack.  The entry is the same for the whole workgroup and is read once, and whether there are
//               rates is the same for the whole launch: without them no rate is loaded.  The stations' rows (S <= 64), one lane
//               each, go to LDS and out as int32 [stack][S]; then the P <= 2016 differences row[j] - row[i], strided over the
//               workgroup in tdoa_locate_set_clock's pair order, go out as long long [stack][P], and beside them U_loc x the
//               differences for the searches on upsampled surfaces.  Plain vector stores.
//
// The host checks the entries (the sources' numbers, |x| <= 65535, 0 <= wa, wb, 1 <= wa + wb <= 65536) and, where there are
// rates, that every continued clock fits int32: by the search's bound on |centre|, the gate, the drift and the largest |x|, or
// word by word where the words are the caller's.  |T| <= 2^16 2^31 and the mean is a convex combination of two such clocks, so
// |row| <= max |cont| and no value on the device needs a check.  clock_mix_row is tdoa_clock_mix_rows' and tdoa_line_mix_rows'
// too, line_cont tdoa_line_mix_rows' and tdoa_sync_line_clock16's.
#pragma once

#include "stack_locate.hpp"

namespace tdoa {

constexpr int kLineMixThreads = 256;
constexpr int kLineMixMaxX = 65535;
constexpr int kClockMixMaxDen = 1 << 16;

// tdoa_line_mix; tdoa_clock_mix's (a, b, wa, wb) with xa = xb = 0
struct LineMix {
    int32_t a, xa, b, xb, wa, wb;
};

__host__ __device__ inline int32_t clock_mix_row(int32_t ca, int32_t cb, int32_t wa, int32_t wb)
{
    const long long den = (long long)wa + wb, T = (long long)wa * ca + (long long)wb * cb;
    const long long r = (2 * (T < 0 ? -T : T) + den) / (2 * den);
    return (int32_t)(T < 0 ? -r : r);
}

// a fine line's clock continued to position x, 1/16 sample: clock16 + r(16 rate x, den), den = U D
__host__ __device__ inline long long line_cont(int32_t clock16, int32_t rate, long long x, long long den)
{
    const long long num = (long long)kLocateDelayUnit * rate * x;
    const long long r = (2 * (num < 0 ? -num : num) + den) / (2 * den);
    return (long long)clock16 + (num < 0 ? -r : r);
}

// word i of the sources at position x: continued where there are rates (the host has seen that it fits), as it is where not
__host__ __device__ inline int32_t line_mix_source(const int32_t *c16, const int32_t *rate, size_t i, long long x, long long den)
{
    return rate ? (int32_t)line_cont(c16[i], rate[i], x, den) : c16[i];
}

// grid (n_stacks), kLineMixThreads threads.  c16, rate: [source][S], the lines or stacks mix names, rate nullptr: none; mix:
// [stack]; den = U D of the lines; S <= kLocateMaxStations, P = S (S - 1) / 2.  rows [stack][S]; cdiff, cdiff_up [stack][P]:
// row[j] - row[i] and U_loc x it.
__global__ __launch_bounds__(kLineMixThreads) void k_line_mix(const int32_t *c16, const int32_t *rate, const LineMix *mix, int S, int P,
                                                              long long den, int U_loc, int32_t *rows, long long *cdiff, long long *cdiff_up)
{
    __shared__ int32_t row_s[kLocateMaxStations];
    const int t = blockIdx.x, lane = threadIdx.x;
    const LineMix m = mix[t];
    if (lane < S) {
        const int32_t r = clock_mix_row(line_mix_source(c16, rate, (size_t)m.a * S + lane, m.xa, den),
                                        line_mix_source(c16, rate, (size_t)m.b * S + lane, m.xb, den), m.wa, m.wb);
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
