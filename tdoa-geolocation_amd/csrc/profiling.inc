// profiling.inc -- per-kernel timing: event scopes on the stream, and the marks an instrumented step graph is built from.
// Included by tdoa_mi355x.hip after tdoa_ctx.

namespace {

void clear_graph_marks(tdoa_ctx *ctx)
{
    for (auto &m : ctx->graph_marks) {
        if (m.e0) (void)hipEventDestroy(m.e0);
        if (m.e1) (void)hipEventDestroy(m.e1);
    }
    ctx->graph_marks.clear();
}

// next free event of the pool, recorded on the context's stream; -1 on failure
int prof_mark(tdoa_ctx *ctx)
{
    if (ctx->prof_used == ctx->prof_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return -1;
        ctx->prof_pool.push_back(e);
    }
    const int id = (int)ctx->prof_used++;
    if (hipEventRecord(ctx->prof_pool[id], ctx->stream) != hipSuccess) return -1;
    return id;
}

// Per-kernel timing of the profiling path: consecutive scopes share the event between them (the stop of one is the
// start of the next), so a step costs one event per kernel boundary; the few microseconds between two kernels count
// towards the later one.  Work enqueued outside any scope must reset ctx->prof_last first.
struct ProfScope {
    tdoa_ctx *ctx;
    ProfRec rec{};
    bool on;
    int mark = -1;                           // graph mode: index into ctx->graph_marks
    static hipGraphNode_t capture_tail(tdoa_ctx *c)
    {
        hipStreamCaptureStatus stt;
        const hipGraphNode_t *deps = nullptr;
        size_t nd = 0;
        if (hipStreamGetCaptureInfo_v2(c->stream, &stt, nullptr, nullptr, &deps, &nd) != hipSuccess || nd != 1) return nullptr;
        return deps[0];
    }
    ProfScope(tdoa_ctx *c, int kernel, double bytes) : ctx(c), on(c->profiling)
    {
        if (c->graph_prof && c->capturing && ((c->prof_mask >> kernel) & 1u)) {
            tdoa_ctx::GraphMark m{kernel, bytes, capture_tail(c), nullptr, nullptr, nullptr};
            if (m.before) {
                mark = (int)c->graph_marks.size();
                c->graph_marks.push_back(m);
            }
        }
        if (on && !((c->prof_mask >> kernel) & 1u)) {      // not selected: its launches are unscoped work
            on = false;
            c->prof_last = -1;
        }
        if (!on) return;
        rec.kernel = kernel;
        rec.bytes = bytes;
        rec.e0 = ctx->prof_last >= 0 ? ctx->prof_last : prof_mark(ctx);
        if (rec.e0 < 0) on = false;
    }
    ~ProfScope()
    {
        if (mark >= 0) ctx->graph_marks[mark].last = capture_tail(ctx);
        if (!on) return;
        rec.e1 = prof_mark(ctx);
        ctx->prof_last = rec.e1;
        if (rec.e1 >= 0) ctx->recs.push_back(rec);
    }
};

void prof_collect(tdoa_ctx *ctx)
{
    for (auto &r : ctx->recs) {
        float ms = 0;
        if (hipEventSynchronize(ctx->prof_pool[r.e1]) == hipSuccess &&
            hipEventElapsedTime(&ms, ctx->prof_pool[r.e0], ctx->prof_pool[r.e1]) == hipSuccess) {
            ctx->prof_ms[r.kernel] += ms;
            ctx->prof_launches[r.kernel] += 1;
            ctx->prof_bytes[r.kernel] += r.bytes;
        }
    }
    ctx->recs.clear();
    ctx->prof_used = 0;
    ctx->prof_last = -1;
}

}  // namespace
