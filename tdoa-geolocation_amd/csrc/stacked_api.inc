// stacked_api.inc -- stacked correlation, host side: the stacks' geometry (StackGeom: the one place their lengths and counts
// are worked out), the stacks of a job, the finishing kernels' launches and downloads (shared by a context's own step,
// step_products.inc, and the group's merged sum), tdoa_num_stacks, and finish_from_host: a merged sum uploaded and handed to
// the stack's finish or to a search on the sums (search_from_host, stack_search.inc).
// Included by tdoa_mi355x.hip after step_graph.inc and before step_products.inc.

extern "C" {

// The stacks of a block of wpb windows, windows_per_stack at a time (0 or more than wpb: the whole block): every length,
// count and index the host code needs of them comes from here.
struct StackGeom {
    int wpb = 0, mm = 0, spb = 0, n_stacks = 0;            // windows per block, windows of a full stack, stacks per block, stacks of the three blocks
    int n_w(int sid) const { return std::min(mm, wpb - (sid % spb) * mm); }        // the last stack of a block may be short
    int stack_of(int wid) const { return (wid / wpb) * spb + (wid % wpb) / mm; }
    int pos_of(int wid) const { return (wid % wpb) % mm; }                          // window wid's place in its stack
};
static StackGeom stack_geom(int wpb, int windows_per_stack)
{
    StackGeom g;
    g.wpb = wpb;
    g.mm = windows_per_stack > 0 ? std::min(windows_per_stack, wpb) : wpb;
    g.spb = (wpb + g.mm - 1) / g.mm;
    g.n_stacks = 3 * g.spb;
    return g;
}

// The stacks of a job (include/tdoa_mi355x.h, "stacked correlation") and which of a rank's pair-windows each (stack, pair)
// sums -- plain numbers, like StepLayout.  The device copy (ctx->stack_desc) is roots, ones, desc, list in this order.
struct StackLayout : StackGeom {
    std::vector<double> roots;               // [n_stacks]: sqrt(n_w)
    std::vector<StackDesc> desc;             // [n_stacks * P]
    std::vector<int32_t> list;               // the rank's pair-window numbers (indices into StepLayout::pw), by stack-pair
};

static StackLayout build_stack_layout(const std::vector<PWDesc> &pw, const StackGeom &geom, int P)
{
    StackLayout L;
    static_cast<StackGeom &>(L) = geom;
    for (int sid = 0; sid < L.n_stacks; sid++) L.roots.push_back(std::sqrt((double)L.n_w(sid)));
    auto stack_pair = [&](const PWDesc &d) { return L.stack_of(d.out_index / P) * P + d.out_index % P; };
    L.desc.assign((size_t)L.n_stacks * P, StackDesc{0, 0});
    for (const PWDesc &d : pw) L.desc[stack_pair(d)].count++;
    int32_t at = 0;
    for (StackDesc &d : L.desc) {
        d.first = at;
        at += d.count;
        d.count = 0;
    }
    L.list.resize(pw.size());
    for (size_t i = 0; i < pw.size(); i++) {
        StackDesc &d = L.desc[stack_pair(pw[i])];
        L.list[d.first + d.count++] = (int32_t)i;
    }
    return L;
}

// the device views of ctx->stack_desc for n_stacks stacks of P pairs
struct StackDev {
    const double *roots, *ones;
    const StackDesc *desc;
    const int32_t *list;
};
static size_t stack_desc_bytes(size_t n_stacks, size_t P, size_t n_owned)
{
    return sizeof(double) * (n_stacks + n_stacks * P) + sizeof(StackDesc) * n_stacks * P + sizeof(int32_t) * std::max<size_t>(n_owned, 1);
}
static StackDev stack_dev(const tdoa_ctx *ctx, size_t n_stacks, size_t P)
{
    StackDev d;
    d.roots = ctx->stack_desc.as<const double>();
    d.ones = d.roots + n_stacks;
    d.desc = reinterpret_cast<const StackDesc *>(d.ones + n_stacks * P);
    d.list = reinterpret_cast<const int32_t *>(d.desc + n_stacks * P);
    return d;
}

// roots and unit scales, and with `runs` the stack-pairs' runs and the list, to ctx->stack_desc; the caller synchronises
// before the host vectors go.  (without `runs` the part a cached step graph's k_stack_accumulate reads stays as it is)
static int upload_stack_desc(tdoa_ctx *ctx, const StackLayout &sl, int P, std::vector<double> *ones, bool runs)
{
    const size_t n_sp = (size_t)sl.n_stacks * P;
    const StackDev d = stack_dev(ctx, sl.n_stacks, P);
    ones->assign(n_sp, 1.0);
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(const_cast<double *>(d.roots), sl.roots.data(), sizeof(double) * sl.n_stacks, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(const_cast<double *>(d.ones), ones->data(), sizeof(double) * n_sp, hipMemcpyHostToDevice, st));
    if (runs && !sl.desc.empty())
        HIPCHK(ctx, hipMemcpyAsync(const_cast<StackDesc *>(d.desc), sl.desc.data(), sizeof(StackDesc) * n_sp, hipMemcpyHostToDevice, st));
    if (runs && !sl.list.empty())
        HIPCHK(ctx, hipMemcpyAsync(const_cast<int32_t *>(d.list), sl.list.data(), sizeof(int32_t) * sl.list.size(), hipMemcpyHostToDevice, st));
    return TDOA_OK;
}

// the buffers of the finishing kernels for n_sp stack-pairs of n_lags lags
static int ensure_stack_finish(tdoa_ctx *ctx, size_t n_sp, int n_lags, int k)
{
    int rc;
    if ((rc = ensure(ctx, ctx->stack_surf, sizeof(float) * n_sp * n_lags))) return rc;
    if ((rc = ensure(ctx, ctx->stack_keys, sizeof(unsigned long long) * n_sp))) return rc;
    if ((rc = ensure(ctx, ctx->stack_fine, sizeof(FineOut) * n_sp))) return rc;
    if ((rc = ensure(ctx, ctx->sel_peaks, sizeof(PeakOut) * n_sp * k))) return rc;
    return ensure(ctx, ctx->sel_count, sizeof(int32_t) * (n_sp + 1));
}

// Q (ctx->stack_q) -> float surfaces, k peaks and the refined peak 1 of every stack-pair: the one place the scale, the
// selection and the refinement of a stack are computed, for a context's own sum and for a group's merged one alike.
// Kernel launches only (the step graph captures them).
static void launch_stack_finish(tdoa_ctx *ctx, int n_stacks, int P, int n_lags, int lag_lo, int k, int min_sep, double gate)
{
    hipStream_t st = ctx->stream;
    const unsigned n_sp = (unsigned)(n_stacks * P);
    const StackDev d = stack_dev(ctx, n_stacks, P);
    auto *Q = ctx->stack_q.as<const long long>();
    auto *keys = ctx->stack_keys.as<unsigned long long>();
    auto *surf = ctx->stack_surf.as<float>();
    auto *peaks = ctx->sel_peaks.as<PeakOut>();
    auto *count = ctx->sel_count.as<int32_t>();
    const dim3 grid(n_sp, (unsigned)((n_lags + kStackTile - 1) / kStackTile));
    hipLaunchKernelGGL(k_zero_u64, dim3((n_sp + 255) / 256), dim3(256), 0, st, keys, (size_t)n_sp);
    hipLaunchKernelGGL(k_stack_finish, grid, dim3(kStackThreads), 0, st, Q, n_lags, lag_lo, P, d.roots, surf, keys);
    hipLaunchKernelGGL(k_select_peaks, dim3(n_sp), dim3(kSelThreads), 0, st, static_cast<const float *>(surf), (size_t)n_lags, n_lags,
                       lag_lo, static_cast<const PWDesc *>(nullptr), static_cast<const unsigned long long *>(keys), d.ones,
                       static_cast<const double *>(nullptr), k, min_sep, peaks, count);
    hipLaunchKernelGGL(k_stack_fine, dim3((n_sp + 63) / 64), dim3(64), 0, st, Q, n_lags, lag_lo, P, (int)n_sp, d.roots,
                       static_cast<const unsigned long long *>(keys), k, peaks, static_cast<const int32_t *>(count),
                       ctx->stack_fine.as<FineOut>(), gate);
}

// the outputs of a finished stack to the host (any pointer may be NULL); asynchronous on ctx->stream
static int download_stack(tdoa_ctx *ctx, size_t n_sp, int n_lags, int k, tdoa_peak *peaks, int32_t *count, tdoa_fine_peak *fine,
                          float *surface)
{
    hipStream_t st = ctx->stream;
    if (peaks) HIPCHK(ctx, hipMemcpyAsync(peaks, ctx->sel_peaks.p, sizeof(PeakOut) * n_sp * k, hipMemcpyDeviceToHost, st));
    if (count) HIPCHK(ctx, hipMemcpyAsync(count, ctx->sel_count.p, sizeof(int32_t) * n_sp, hipMemcpyDeviceToHost, st));
    if (fine) HIPCHK(ctx, hipMemcpyAsync(fine, ctx->stack_fine.p, sizeof(FineOut) * n_sp, hipMemcpyDeviceToHost, st));
    if (surface) HIPCHK(ctx, hipMemcpyAsync(surface, ctx->stack_surf.p, sizeof(float) * n_sp * n_lags, hipMemcpyDeviceToHost, st));
    return TDOA_OK;
}

int tdoa_num_stacks(const tdoa_ctx *ctx, int windows_per_stack, int *stacks_per_block, int *n_stacks_total)
{
    if (!ctx || windows_per_stack < 0) return TDOA_ERR_INVALID;
    int wpb = 0;
    const int rc = tdoa_num_windows(ctx, &wpb, nullptr);
    if (rc) return rc;
    const StackGeom g = stack_geom(wpb, windows_per_stack);
    if (stacks_per_block) *stacks_per_block = g.spb;
    if (n_stacks_total) *n_stacks_total = g.n_stacks;
    return TDOA_OK;
}

// the arguments of tdoa_process_stacked / tdoa_group_process_stacked that need no device
static const char *check_stacked_args(int windows_per_stack, int k, int min_separation, double gate_samples, bool any_output)
{
    if (windows_per_stack < 0) return "windows_per_stack < 0";
    if (const char *bad = check_k_sep(k, min_separation)) return bad;
    if (!(gate_samples >= 0.0)) return "gate < 0";
    if (!any_output) return "every output is NULL";
    return nullptr;
}

// The end of every call that launches outside a step graph: the launches' error, the call's own copies out, the wait (the
// host vectors its uploads read go after it).
static int download_and_wait(tdoa_ctx *ctx, const std::function<int()> &download)
{
    HIPCHK(ctx, hipGetLastError());
    if (int rc = download()) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TDOA_OK;
}

// A group's merged sum on one context: q_sum into ctx->stack_q with the stacks' roots and unit scales beside it, then
// launch(n_stacks, roots) -- the caller's own buffers and the kernels a context's own call ends with -- and its download.
// Not part of a step graph (the context's cached step stays valid unless a buffer had to grow: the runs and the list its
// k_stack_accumulate reads stay as they are).
static int finish_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack,
                            const std::function<int(int n_stacks, const double *roots)> &launch,
                            const std::function<int(int n_stacks)> &download)
{
    int rc, wpb = 0;
    if ((rc = check_ctx(ctx))) return rc;
    if ((rc = tdoa_num_windows(ctx, &wpb, nullptr))) return fail(ctx, rc, "captures missing or too small");
    const int P = tdoa_num_pairs(ctx), n_lags = 2 * ctx->prm.max_lag - 1;
    const StackLayout sl = build_stack_layout({}, stack_geom(wpb, windows_per_stack), P);
    const size_t n_sp = (size_t)sl.n_stacks * P;
    if ((rc = ensure(ctx, ctx->stack_q, sizeof(long long) * n_sp * n_lags))) return rc;
    if ((rc = ensure(ctx, ctx->stack_desc, stack_desc_bytes(sl.n_stacks, P, 0)))) return rc;   // (a member's step made it larger)
    std::vector<double> ones;
    if ((rc = upload_stack_desc(ctx, sl, P, &ones, false))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->stack_q.p, q_sum, sizeof(int64_t) * n_sp * n_lags, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch(sl.n_stacks, stack_dev(ctx, sl.n_stacks, P).roots))) return rc;
    return download_and_wait(ctx, [&] { return download(sl.n_stacks); });
}

// the merged stacks finished: surfaces, k peaks and the refined peak 1
static int stack_finish_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack, int k, int min_separation,
                                  double gate, tdoa_peak *peaks, int32_t *count, tdoa_fine_peak *fine, float *surface)
{
    const int P = tdoa_num_pairs(ctx), n_lags = 2 * ctx->prm.max_lag - 1, lag_lo = -(ctx->prm.max_lag - 1);
    return finish_from_host(
        ctx, q_sum, windows_per_stack,
        [&](int n_stacks, const double *) -> int {
            if (int rc = ensure_stack_finish(ctx, (size_t)n_stacks * P, n_lags, k)) return rc;
            launch_stack_finish(ctx, n_stacks, P, n_lags, lag_lo, k, min_separation, gate);
            return TDOA_OK;
        },
        [&](int n_stacks) { return download_stack(ctx, (size_t)n_stacks * P, n_lags, k, peaks, count, fine, surface); });
}

}  // extern "C"
