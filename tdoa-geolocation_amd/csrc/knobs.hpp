// knobs.hpp -- the library's path switches: the table of them, and how a context reads it.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "../../include/tdoa_mi355x.h"

namespace {

// Path switches (A/B measurements, tests): read from the environment once, when the context is made -- a captured graph
// must not depend on an environment that changes later --, partly rewritten by tdoa_debug_flags / tdoa_debug_force_generic.
// kKnobVars says what each one does.  Every field is an element of the step graph's key.
struct Knobs {
    bool force_generic = false, use_graph = true, short_lag = true, segment_form = true, segment_quads = true, decimate = true,
         k1_once = true, pow2_only = false, fused_k1 = true, dec_cols = true, dec_cols_always = false, dec_staged = true,
         small_fused = true, small_fused_always = false, stg_folded = true, stg_folded_always = false, stg_blocks = true,
         seg_pack3 = true, memset_nodes = false, xcd_rows = true, stg_merge = true, k1_split = true, k1_split_512 = false,
         stg_paired = true, stg_nt = true;
    int zpad = 256, stg_loaders = 0, stg_rows = 0, stg_cw = 0, stg_bufs = 0, seg_chunks_override = 0, xcd_pair_mb = 48;
};

// One row per Knobs field: its environment variable (nullptr: none) and how a value is read -- a switch takes `when_one`
// where the value starts with '1' and the opposite otherwise, a number is clamp(atoi(value)) --, and the tdoa_debug_flags
// bit that sets a switch (TDOA_DEBUG_*, 0: none) the same way: `when_one` where it is set, the opposite where it is not
struct KnobVar {
    const char *env;
    unsigned int debug_bit;
    bool Knobs::*flag;
    bool when_one;
    int Knobs::*num;
    int (*clamp)(int);
};
constexpr KnobVar off_if(const char *env, bool Knobs::*f, unsigned int bit = 0) { return {env, bit, f, false, nullptr, nullptr}; }
constexpr KnobVar on_if(const char *env, bool Knobs::*f, unsigned int bit = 0) { return {env, bit, f, true, nullptr, nullptr}; }
constexpr KnobVar number(const char *env, int Knobs::*f, int (*clamp)(int)) { return {env, 0, nullptr, false, f, clamp}; }
const KnobVar kKnobVars[] = {
    on_if(nullptr, &Knobs::force_generic, TDOA_DEBUG_GENERIC_KERNELS),                 // tests: the any-size kernels even at the hot sizes
    off_if("TDOA_NO_GRAPH", &Knobs::use_graph),            // no whole-step hipGraph
    off_if("TDOA_NO_SHORT_LAG", &Knobs::short_lag, TDOA_DEBUG_NO_SHORT_LAG),        // the general inverse for short searches
    off_if("TDOA_NO_SEGMENT_FORM", &Knobs::segment_form, TDOA_DEBUG_NO_SEGMENT_FORM),  // no LDS-resident overlap-save form for short searches
    off_if("TDOA_NO_SEGMENT_QUADS", &Knobs::segment_quads, TDOA_DEBUG_NO_SEGMENT_QUADS),      // segment form one pair-window at a time (no shared station transforms)
    off_if("TDOA_NO_DECIMATE", &Knobs::decimate, TDOA_DEBUG_NO_DECIMATE),          // the full inverse even where the decimated one applies
    off_if("TDOA_NO_K1_ONCE", &Knobs::k1_once, TDOA_DEBUG_NO_K1_ONCE),            // the statistics pre-pass everywhere (no single-look K1, k1_single_look.hpp)
    on_if("TDOA_POW2_ONLY", &Knobs::pow2_only, TDOA_DEBUG_POW2_ONLY),            // transform lengths are powers of two everywhere (no 5 x 2^22 plan for ten-second windows)
    // padding (elements) after every 256 rows of a two-sweep plan's TZ: 2 KB; measured on cfg3: 0 -> 107 ms column pass, 128 -> 91,
    // 256 -> 87, 512 -> 89.  Rows stay 128-byte aligned (the finish sweep reads 16-byte pairs).
    number("TDOA_ZPAD", &Knobs::zpad, [](int v) { return v < 0 ? 0 : v > 4096 ? 4096 : v & ~15; }),
    off_if("TDOA_NO_FUSED_K1", &Knobs::fused_k1, TDOA_DEBUG_NO_FUSED_K1),          // K1 always materialises its codes (no discriminator inside the column kernels)
    off_if("TDOA_NO_DEC_COLS", &Knobs::dec_cols, TDOA_DEBUG_NO_DEC_COLS),          // the tile form of the decimated pair step (k_pair_decimate16; none on 4096 x 4096 plans)
    on_if("TDOA_DEC_COLS_ALWAYS", &Knobs::dec_cols_always, TDOA_DEBUG_DEC_COLS_ALWAYS),      // the column walk wherever the decimated inverse applies (measurements)
    off_if("TDOA_NO_DEC_STAGED", &Knobs::dec_staged, TDOA_DEBUG_NO_DEC_STAGED),      // the column walk one pair-window per wave from memory (k_pair_decimate_cols), no LDS staging
    off_if("TDOA_NO_SMALL_FUSED", &Knobs::small_fused, TDOA_DEBUG_NO_SMALL_FUSED),    // the decimated inverse's small plan as two kernels with V' in memory between them
    on_if("TDOA_SMALL_FUSED_ALWAYS", &Knobs::small_fused_always, TDOA_DEBUG_SMALL_FUSED_ALWAYS),      // ... fused for any number of pair-windows (tests)
    off_if("TDOA_NO_STG_FOLDED", &Knobs::stg_folded),      // the staged walk always with a loader wave next to at most fifteen walks
    on_if("TDOA_STG_FOLDED_ALWAYS", &Knobs::stg_folded_always),      // ... folded wherever the blocked layout applies (tests)
    off_if("TDOA_NO_STG_BLOCKS", &Knobs::stg_blocks),      // the staged walk reads row-major spectra on every plan
    // the blocked plans' spectra as [column / 64][k2][column % 64] (two 512-byte pieces per LDS-DMA) instead of the paired lines of
    // stg_paired_at (dec_staged.hpp)
    off_if("TDOA_NO_STG_PAIRED", &Knobs::stg_paired),
    // the loader wave's LDS-DMA with the default cache policy even where a launch reads every staged byte once (one pair group)
    off_if("TDOA_NO_STG_NT", &Knobs::stg_nt),
    off_if("TDOA_NO_STG_MERGE", &Knobs::stg_merge),        // the staged walk leaves every column's neighbour shares in X for the small plan's row pass
    // loader waves per workgroup of k_pair_decimate_staged, rows per phase, at most n walks (compute waves) per workgroup, phases
    // in the LDS ring (0: the library's choice)
    number("TDOA_DEC_STAGED_LOADERS", &Knobs::stg_loaders, [](int v) { return std::max(0, std::min(4, v)); }),
    number("TDOA_DEC_STAGED_ROWS", &Knobs::stg_rows, [](int v) { return v == 8 || v == 4 || v == 2 ? v : 0; }),
    number("TDOA_DEC_STAGED_CW", &Knobs::stg_cw, [](int v) { return std::max(0, std::min(15, v)); }),
    number("TDOA_DEC_STAGED_BUFS", &Knobs::stg_bufs, [](int v) { return std::max(0, std::min(16, v)); }),
    off_if("TDOA_NO_SEG_PACK3", &Knobs::seg_pack3, TDOA_DEBUG_NO_SEG_PACK3),        // the segment form reads int32 code rows (round 3's layout)
    number("TDOA_SEG_CHUNKS", &Knobs::seg_chunks_override, [](int v) { return std::max(0, v); }),      // chunk count of the segment form
    // probe only: zero the step's accumulators with hipMemsetAsync nodes instead of k_zero_u64 kernel nodes
    on_if("TDOA_DEBUG_MEMSET_NODES", &Knobs::memset_nodes),
    off_if("TDOA_NO_XCD_ROWS", &Knobs::xcd_rows, TDOA_DEBUG_NO_XCD_ROWS),          // plain 2-D grid of the pair kernels even with more pairs than stations
    // k_pair_decimate16 groups a window's pair-windows on one XCD when the window's spectra exceed n MB (round 4, same-box A/B:
    // cfg4, 8 x 8.4 MB, 11.05 ms grouped against 11.20 -- its pair step pulled 27 GB per step through the fabric for 5.6 GB of
    // spectra; cfg2, 3 x 8.4 MB: 0.69 ms grouped against 0.66 plain)
    number("TDOA_XCD_PAIR_MB", &Knobs::xcd_pair_mb, [](int v) { return std::max(0, v); }),
    // the fused column kernels look angles up in the 64 KB quadrant table (22 vector instructions per dword) instead of the 96 KB
    // split half-plane table (11; k1_discriminator.hpp) -- also what a device without 160 KB of LDS per workgroup runs
    off_if("TDOA_K1_QUAD_TABLE", &Knobs::k1_split),
    // ... the split table in k_fwd_col512_k1 too.  Off by default: that kernel exchanges through LDS twice per tile and the
    // extra gathers cost more than the instructions save (cfg5 step 151.9 -> 154.3 ms, profiles/r07_k1_split_ab.json)
    on_if("TDOA_K1_SPLIT_512", &Knobs::k1_split_512),
};

// run-time switches are read ONCE, when the context is made (a captured graph must not depend on an environment that changes later)
inline void knobs_from_env(Knobs &k)
{
    for (const KnobVar &kv : kKnobVars) {
        const char *e = kv.env ? std::getenv(kv.env) : nullptr;
        if (!e) continue;
        if (kv.flag) k.*kv.flag = e[0] == '1' ? kv.when_one : !kv.when_one;
        else k.*kv.num = kv.clamp(std::atoi(e));
    }
}

// tdoa_debug_flags: every switch with a TDOA_DEBUG_* bit is set from `flags`
inline void knobs_from_debug_flags(Knobs &k, unsigned int flags)
{
    for (const KnobVar &kv : kKnobVars)
        if (kv.debug_bit) k.*kv.flag = (flags & kv.debug_bit) ? kv.when_one : !kv.when_one;
}

}  // namespace
