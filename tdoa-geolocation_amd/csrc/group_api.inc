// group_api.inc -- the multi-device group (include/tdoa_mi355x.h, "multi-device group"): one tdoa_ctx per member, member k
// is rank k of n_members, and one call shards tdoa_process over them and merges their peak records on the host
// (tdoa_process_stacked: adds their fixed-point partial sums and finishes the sum on member 0).
// Included by tdoa_mi355x.hip after its entries and before stack_search.inc; uses its helpers (fail, check_ctx, unit_owner,
// capture_upload_file_runs).  The group's calls of the searches on the stacks' sums are in the searches' own files
// (group_process_search, stack_search.inc).
//
// Threads.  tdoa_group_capture_upload_files and tdoa_group_process run member 0 on the caller's thread and members 1..n-1
// on std::threads started for the call; each thread calls into its own context only.  Two conditions make that safe, and a
// change to either breaks the group:
//  * every entry point a member thread calls sets ctx->device on that thread itself (check_ctx, tdoa_capture_clear): a new
//    thread starts on device 0, and the caller's thread is left on whatever device the last context it used had;
//  * the step graph is captured with hipStreamCaptureModeThreadLocal (run_step_graph): a member capturing its step does
//    not turn the HIP calls another member makes at the same time (hipMalloc, synchronous copies) into capture errors, as
//    the global capture mode would.
// Members that share a GPU size their launch groups from hipMemGetInfo at call time (batch_bound) while the others hold
// memory too, so their groupings can differ from one call to the next; every grouping gives the same peaks.
//
// No collective: every member's tdoa_process already copies its W x P peak records to the host, which is where the caller
// wants the result, so the merge is a host loop over the records (DESIGN.md section 7).

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <thread>

struct tdoa_group {
    std::vector<tdoa_ctx *> members;
    std::vector<std::vector<tdoa_peak>> out;  // member k's tdoa_process(k, n) records, kept from call to call
    std::vector<std::vector<int64_t>> partial;   // member k's tdoa_process_stacked(k, n) sums, likewise
    std::string last_error;
};

namespace {

thread_local std::string g_group_create_error;   // tdoa_group_last_error(NULL): this thread's last failed tdoa_group_create

using SampleRun = std::pair<size_t, size_t>;     // first sample, sample count

// sharding.owned_sample_runs: the runs of a capture of `total` samples that tdoa_process(rank, world) reads, the window
// grid taken from the shortest capture of the job (n_min) and the block offsets from the capture's own thirds.  Adjacent
// owned windows merge into one run; in the pair-major fallback a rank may need any window, so the whole capture is one run.
// false: more windows than an int counts.
bool owned_sample_runs(size_t total, size_t n_min, long long window_len, int rank, int world, std::vector<SampleRun> *runs)
{
    runs->clear();
    const size_t block = total / 3, bmin = n_min / 3;
    const size_t wlen = std::min<size_t>((size_t)window_len, bmin);
    if (wlen && bmin / wlen > (1u << 28)) return false;
    const int wpb = wlen ? (int)std::max<size_t>(1, bmin / wlen) : 0;
    const int W = 3 * wpb;
    if (W < world) {
        runs->emplace_back(0, total);
        return true;
    }
    for (int wid = 0; wid < W; wid++) {
        if (unit_owner(wid, 0, W, 1, world) != rank) continue;      // window-major: every pair of wid on one rank
        const size_t first = (size_t)(wid / wpb) * block + (size_t)(wid % wpb) * wlen;
        if (!runs->empty() && runs->back().first + runs->back().second == first)
            runs->back().second += wlen;
        else
            runs->emplace_back(first, wlen);
    }
    return true;
}

int group_fail(tdoa_group *g, int status, const std::string &what)
{
    g->last_error = what;
    return status;
}

std::string member_name(int k, int device)
{
    return "member " + std::to_string(k) + " (device " + std::to_string(device) + "): ";
}

// status of member k's failed call, its context's tdoa_last_error named after the member
int member_fail(tdoa_group *g, int k, int status)
{
    const tdoa_ctx *c = g->members[k];
    const char *detail = c->last_error.empty() ? tdoa_strerror(status) : c->last_error.c_str();
    return group_fail(g, status, member_name(k, c->device) + detail);
}

// work(k) for every member: member 0 on the caller's thread, the others on threads of their own, all joined on return.
// false: a thread could not be started (the members that did start have run and been joined; member 0 has not run).
bool run_members(int n, const std::function<void(int)> &work)
{
    std::vector<std::thread> pool;
    bool started = true;
    try {
        for (int k = 1; k < n; k++) pool.emplace_back(work, k);
    } catch (...) {
        started = false;
    }
    if (started) work(0);
    for (auto &t : pool) t.join();
    return started;
}

// The merges take (window, pair) records and sums from different members: they must all cut the same windows of the same
// stations.  false: *who is the first member whose station count or capture lengths differ from member 0's.
bool group_same_captures(const tdoa_group *g, int *who)
{
    const auto &a = g->members[0]->caps;
    for (int k = 1; k < (int)g->members.size(); k++) {
        const auto &b = g->members[k]->caps;
        bool same = a.size() == b.size();
        for (size_t s = 0; same && s < a.size(); s++) same = a[s].n == b[s].n;
        if (!same) {
            *who = k;
            return false;
        }
    }
    return true;
}

// What the stacked group calls share once their own checks are through: the members' shares of the stacks' fixed-point sums
// (each member's tdoa_process_stacked returns only its partial Q; k = min_separation = 1 and gate 0 reach nothing but its
// step graph's key, so the three calls replay one graph per windows_per_stack), added on the host into member 0's (integer
// addition: any order gives the same words).  *merged stays valid until the group's next call.
int group_merged_q(tdoa_group *g, int windows_per_stack, const int64_t **merged)
{
    const int world = (int)g->members.size();
    tdoa_ctx *c0 = g->members[0];
    if (int who = 0; !group_same_captures(g, &who))
        return group_fail(g, TDOA_ERR_STATE, member_name(who, g->members[who]->device) +
                                                 "station count or capture lengths differ from member 0's");
    int n_stacks = 0;
    if (tdoa_num_stacks(c0, windows_per_stack, nullptr, &n_stacks) != TDOA_OK)
        return group_fail(g, TDOA_ERR_STATE, member_name(0, c0->device) + "captures missing or too small");
    const size_t n_q = (size_t)n_stacks * tdoa_num_pairs(c0) * (size_t)(2 * c0->prm.max_lag - 1);
    g->partial.resize(world);
    for (auto &q : g->partial) q.resize(n_q);
    std::vector<int> status(world, TDOA_OK);
    const bool ran = run_members(world, [&](int m) {
        status[m] = tdoa_process_stacked(g->members[m], m, world, windows_per_stack, 1, 1, 0.0, nullptr, nullptr, nullptr, nullptr,
                                         g->partial[m].data());
    });
    if (!ran) return group_fail(g, TDOA_ERR_NOMEM, "could not start a member thread");
    for (int m = 0; m < world; m++)
        if (status[m] != TDOA_OK) return member_fail(g, m, status[m]);
    std::vector<int64_t> &sum = g->partial[0];
    for (int m = 1; m < world; m++) {
        const int64_t *q = g->partial[m].data();
        for (size_t i = 0; i < n_q; i++) sum[i] += q[i];
    }
    *merged = sum.data();
    return TDOA_OK;
}

// one member's share of the group's file ingest: its previous captures dropped, then every file's owned runs
int group_member_upload(tdoa_ctx *ctx, int rank, int world, const std::vector<int> &fds, const std::vector<size_t> &n_samples,
                        size_t n_min)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if ((rc = tdoa_capture_clear(ctx))) return rc;
    std::vector<SampleRun> runs;
    for (size_t s = 0; s < fds.size(); s++) {
        if (!owned_sample_runs(n_samples[s], n_min, ctx->prm.window_len, rank, world, &runs))
            return fail(ctx, TDOA_ERR_UNSUPPORTED, "too many windows");
        if ((rc = capture_upload_file_runs(ctx, (int)s, fds[s], n_samples[s], runs))) return rc;
    }
    return TDOA_OK;
}

}  // namespace

extern "C" {

int tdoa_group_create(const tdoa_params *p, const int32_t *devices, int n_members, tdoa_group **out)
{
    if (!out) return TDOA_ERR_INVALID;
    *out = nullptr;
    g_group_create_error.clear();
    if (n_members < 1 || !devices) {
        g_group_create_error = "n_members < 1 or devices is NULL";
        return TDOA_ERR_INVALID;
    }
    for (int k = 0; k < n_members; k++)
        if (devices[k] < 0) {
            g_group_create_error = member_name(k, devices[k]) + "negative device ordinal";
            return TDOA_ERR_INVALID;
        }
    const int ndev = tdoa_device_count();
    for (int k = 0; k < n_members; k++)
        if (devices[k] >= ndev) {
            g_group_create_error = member_name(k, devices[k]) + "no such device (tdoa_device_count() = " + std::to_string(ndev) + ")";
            return TDOA_ERR_NO_DEVICE;
        }
    tdoa_params prm;
    if (p)
        prm = *p;
    else
        tdoa_default_params(&prm);
    tdoa_group *g = new (std::nothrow) tdoa_group();
    if (!g) return TDOA_ERR_NOMEM;
    for (int k = 0; k < n_members; k++) {
        prm.device = devices[k];
        tdoa_ctx *c = nullptr;
        const int rc = tdoa_create(&prm, &c);
        if (rc != TDOA_OK) {
            g_group_create_error = member_name(k, devices[k]) + "tdoa_create: " + tdoa_strerror(rc);
            tdoa_group_destroy(g);
            return rc;
        }
        g->members.push_back(c);
    }
    *out = g;
    return TDOA_OK;
}

void tdoa_group_destroy(tdoa_group *g)
{
    if (!g) return;
    for (tdoa_ctx *c : g->members) tdoa_destroy(c);
    delete g;
}

const char *tdoa_group_last_error(const tdoa_group *g) { return g ? g->last_error.c_str() : g_group_create_error.c_str(); }

tdoa_ctx *tdoa_group_member(tdoa_group *g, int k)
{
    return (g && k >= 0 && k < (int)g->members.size()) ? g->members[k] : nullptr;
}

int tdoa_group_capture_upload_files(tdoa_group *g, int n_stations, const char *const *paths, size_t *n_samples)
{
    if (!g) return TDOA_ERR_INVALID;
    if (n_stations < 1 || n_stations > 1024 || !paths) return group_fail(g, TDOA_ERR_INVALID, "bad station count or paths");
    std::vector<int> fds(n_stations, -1);
    std::vector<size_t> n(n_stations, 0);
    auto close_all = [&]() {
        for (int fd : fds)
            if (fd >= 0) close(fd);
    };
    for (int s = 0; s < n_stations; s++) {
        struct stat sb;
        fds[s] = paths[s] ? open(paths[s], O_RDONLY | O_CLOEXEC) : -1;
        if (fds[s] < 0 || fstat(fds[s], &sb) != 0 || sb.st_size < 0) {
            close_all();
            return group_fail(g, TDOA_ERR_INVALID, "station " + std::to_string(s) + ": failed to open " + (paths[s] ? paths[s] : "(NULL)"));
        }
        n[s] = (size_t)sb.st_size / 2;                          // processor.go:182
    }
    const size_t n_min = *std::min_element(n.begin(), n.end());
    const int world = (int)g->members.size();
    std::vector<int> status(world, TDOA_OK);
    const bool ran = run_members(world, [&](int k) { status[k] = group_member_upload(g->members[k], k, world, fds, n, n_min); });
    close_all();
    if (!ran) return group_fail(g, TDOA_ERR_NOMEM, "could not start a member thread");
    for (int k = 0; k < world; k++)
        if (status[k] != TDOA_OK) return member_fail(g, k, status[k]);
    if (n_samples) std::copy(n.begin(), n.end(), n_samples);
    return TDOA_OK;
}

int tdoa_group_process(tdoa_group *g, tdoa_peak *out_host)
{
    if (!g) return TDOA_ERR_INVALID;
    if (!out_host) return group_fail(g, TDOA_ERR_INVALID, "out_host is NULL");
    const int world = (int)g->members.size();
    tdoa_ctx *c0 = g->members[0];
    if (int who = 0; !group_same_captures(g, &who))
        return group_fail(g, TDOA_ERR_STATE, member_name(who, g->members[who]->device) +
                                                 "station count or capture lengths differ from member 0's");
    int wpb = 0, W = 0;
    if (tdoa_num_windows(c0, &wpb, &W) != TDOA_OK)
        return group_fail(g, TDOA_ERR_STATE, member_name(0, c0->device) + "captures missing or too small");
    const int P = tdoa_num_pairs(c0);
    if (world == 1) {                        // no merge, no copy
        const int rc = tdoa_process(c0, 0, 1, out_host, nullptr);
        return rc == TDOA_OK ? rc : member_fail(g, 0, rc);
    }
    const size_t slots = (size_t)W * P;
    g->out.resize(world);
    for (auto &o : g->out) o.resize(slots);
    std::vector<int> status(world, TDOA_OK);
    const bool ran = run_members(world, [&](int k) { status[k] = tdoa_process(g->members[k], k, world, g->out[k].data(), nullptr); });
    if (!ran) return group_fail(g, TDOA_ERR_NOMEM, "could not start a member thread");
    for (int k = 0; k < world; k++)
        if (status[k] != TDOA_OK) return member_fail(g, k, status[k]);
    for (int wid = 0; wid < W; wid++)
        for (int p = 0; p < P; p++) {
            const size_t u = (size_t)wid * P + p;
            out_host[u] = g->out[unit_owner(wid, p, W, P, world)][u];
        }
    return TDOA_OK;
}

// tdoa_process_stacked over the members: the host adds their shares of the fixed-point sums (group_merged_q) and member 0
// finishes the sum with the kernels a single context's call ends with.
int tdoa_group_process_stacked(tdoa_group *g, int windows_per_stack, int k, int min_separation, double gate_samples,
                               tdoa_peak *peaks_host, int32_t *count_host, tdoa_fine_peak *fine_host, float *surface_host)
{
    if (!g) return TDOA_ERR_INVALID;
    if (const char *bad = check_stacked_args(windows_per_stack, k, min_separation, gate_samples,
                                             peaks_host || count_host || fine_host || surface_host))
        return group_fail(g, TDOA_ERR_INVALID, bad);
    const int world = (int)g->members.size();
    tdoa_ctx *c0 = g->members[0];
    if (world == 1) {                        // no merge: the member's call writes the outputs
        const int rc = tdoa_process_stacked(c0, 0, 1, windows_per_stack, k, min_separation, gate_samples, peaks_host, count_host,
                                            fine_host, surface_host, nullptr);
        return rc == TDOA_OK ? rc : member_fail(g, 0, rc);
    }
    if (c0->prm.lag_mode == TDOA_LAGS_GO) return group_fail(g, TDOA_ERR_UNSUPPORTED, "stacked correlation with TDOA_LAGS_GO");
    const int64_t *sum = nullptr;
    if (const int rc = group_merged_q(g, windows_per_stack, &sum)) return rc;
    const int rc = stack_finish_from_host(c0, sum, windows_per_stack, k, min_separation, gate_samples, peaks_host,
                                          count_host, fine_host, surface_host);
    return rc == TDOA_OK ? rc : member_fail(g, 0, rc);
}

// the table to every member: each keeps its own copy, member 0's is the one a group of several searches with
int tdoa_group_locate_set_table(tdoa_group *g, const int32_t *delay, int n_cells, int n_cols, int n_stations)
{
    if (!g) return TDOA_ERR_INVALID;
    for (size_t m = 0; m < g->members.size(); m++)
        if (const int rc = tdoa_locate_set_table(g->members[m], delay, n_cells, n_cols, n_stations)) return member_fail(g, (int)m, rc);
    return TDOA_OK;
}

// the zoom locate's fine table to every member
int tdoa_group_locate_set_fine_table(tdoa_group *g, const int32_t *delay, int n_cells, int n_cols, int n_stations)
{
    if (!g) return TDOA_ERR_INVALID;
    for (size_t m = 0; m < g->members.size(); m++)
        if (const int rc = tdoa_locate_set_fine_table(g->members[m], delay, n_cells, n_cols, n_stations)) return member_fail(g, (int)m, rc);
    return TDOA_OK;
}

// the clocks to every member: each keeps its own copy, member 0's is the one a group of several searches with
int tdoa_group_locate_set_clock(tdoa_group *g, const int32_t *clock, int n_stacks, int n_stations)
{
    if (!g) return TDOA_ERR_INVALID;
    for (size_t m = 0; m < g->members.size(); m++)
        if (const int rc = tdoa_locate_set_clock(g->members[m], clock, n_stacks, n_stations)) return member_fail(g, (int)m, rc);
    return TDOA_OK;
}

int tdoa_group_locate_set_stats(tdoa_group *g, const uint16_t *ranks, int n_ranks, int foot)
{
    if (!g) return TDOA_ERR_INVALID;
    for (size_t m = 0; m < g->members.size(); m++)
        if (const int rc = tdoa_locate_set_stats(g->members[m], ranks, n_ranks, foot)) return member_fail(g, (int)m, rc);
    return TDOA_OK;
}

// the factor to every member: member 0's is the one a group of several searches with, on the merged sum (the upsampler's
// rounding is not linear: upsampling comes after the merge)
int tdoa_group_locate_set_upsample(tdoa_group *g, int U)
{
    if (!g) return TDOA_ERR_INVALID;
    for (size_t m = 0; m < g->members.size(); m++)
        if (const int rc = tdoa_locate_set_upsample(g->members[m], U)) return member_fail(g, (int)m, rc);
    return TDOA_OK;
}

// the statistics of the group's last call of the family: member 0 ran its search, on its own captures or on the merged sum
int tdoa_group_locate_last_stats(tdoa_group *g, tdoa_map_stats *out, int max_planes, int *n_planes)
{
    if (!g) return TDOA_ERR_INVALID;
    const int rc = tdoa_locate_last_stats(g->members[0], out, max_planes, n_planes);
    return rc == TDOA_OK ? rc : member_fail(g, 0, rc);
}

int tdoa_debug_owned_runs(size_t total_samples, size_t n_min, int64_t window_len, int rank, int world, size_t *first,
                          size_t *count, int max_runs, int *n_runs)
{
    if (world < 1 || rank < 0 || rank >= world || window_len < 1 || n_min > total_samples || max_runs < 0 || !n_runs ||
        (max_runs > 0 && (!first || !count)))
        return TDOA_ERR_INVALID;
    std::vector<SampleRun> runs;
    if (!owned_sample_runs(total_samples, n_min, window_len, rank, world, &runs)) return TDOA_ERR_UNSUPPORTED;
    *n_runs = (int)runs.size();
    for (int i = 0; i < max_runs && i < (int)runs.size(); i++) {
        first[i] = runs[i].first;
        count[i] = runs[i].second;
    }
    return TDOA_OK;
}

}  // extern "C"
