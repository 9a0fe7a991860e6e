// stack_clock_mix.hpp -- tdoa_process_sync_locate's middle link (include/tdoa_mi355x.h, "clocks to fix in one call"): the
// clock row of every stack, made on the device from the fine clock search's clocks (stack_sync_fine.hpp), and the pairs'
// clock differences the delay-table family's kernels take as cdiff (stack_locate.hpp).  Which stacks' clocks make which
// stack's row is data: mix[t] = (a, b, wa, wb), and for station s, in 64 bits,
//     T = wa c16[a][s] + wb c16[b][s]      row[t][s] = sgn(T) ((2 |T| + den) div (2 den)),  den = wa + wb
// the nearest integer to T / den, halves away from zero.  (t, t, 1, 0) is the stack's own clock; (a, b, 1, 1) is the
// midpoint rule (|T| + 1) div 2.  The sum is rounded, not an increment: on exact halves of opposite sign this differs from
// a ramp that rounds its steps.  The kernel knows nothing about blocks.
//
// k_clock_mix   one workgroup per stack.  a, b, wa, wb are the same for the whole workgroup and are read once.  The stations'
//               rows (S <= 64), one lane each, go to LDS and out as int32 [stack][S]; then the P <= 2016 differences
//               row[j] - row[i], strided over the workgroup in tdoa_locate_set_clock's pair order, go out as long long
//               [stack][P], and beside them U x the differences for the searches on upsampled surfaces.  Plain vector stores.
//
// The host checks the weights (0 <= wa, wb, 1 <= den <= 65536) and the stacks' numbers: |T| <= 2^16 2^31, a convex
// combination, so |row| <= max |c16| and no value on the device needs a check.  clock_mix_row is tdoa_clock_mix_rows' too.
#pragma once

#include "stack_locate.hpp"

namespace tdoa {

constexpr int kClockMixThreads = 256;
constexpr int kClockMixMaxDen = 1 << 16;

// tdoa_clock_mix
struct ClockMix {
    int32_t a, b, wa, wb;
};

__host__ __device__ inline int32_t clock_mix_row(int32_t ca, int32_t cb, int32_t wa, int32_t wb)
{
    const long long den = (long long)wa + wb, T = (long long)wa * ca + (long long)wb * cb;
    const long long r = (2 * (T < 0 ? -T : T) + den) / (2 * den);
    return (int32_t)(T < 0 ? -r : r);
}

// grid (n_stacks), kClockMixThreads threads.  c16: [stack][S], the stacks mix names; mix: [stack]; S <= kLocateMaxStations,
// P = S (S - 1) / 2.  rows [stack][S]; cdiff, cdiff_up [stack][P]: row[j] - row[i] and U x it.
__global__ __launch_bounds__(kClockMixThreads) void k_clock_mix(const int32_t *c16, const ClockMix *mix, int S, int P, int U, int32_t *rows,
                                                                long long *cdiff, long long *cdiff_up)
{
    __shared__ int32_t row_s[kLocateMaxStations];
    const int t = blockIdx.x, lane = threadIdx.x;
    const ClockMix m = mix[t];
    if (lane < S) {
        const int32_t r = clock_mix_row(c16[(size_t)m.a * S + lane], c16[(size_t)m.b * S + lane], m.wa, m.wb);
        row_s[lane] = r;
        rows[(size_t)t * S + lane] = r;
    }
    __syncthreads();
    for (int p = lane; p < P; p += kClockMixThreads) {
        int i, j;
        locate_pair(p, S, &i, &j);
        const long long d = (long long)row_s[j] - (long long)row_s[i];
        cdiff[(size_t)t * P + p] = d;
        cdiff_up[(size_t)t * P + p] = d * U;
    }
}

}  // namespace tdoa
