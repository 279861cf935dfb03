// ctx.hip -- context lifecycle, memory, copies, profiling, the side stream, device queries.  (Binding a data set: bind.hip.)
#include <cstdarg>
#include <cstdlib>

#include "common.h"
#include <algorithm>
#include <chrono>
#include <mutex>

static std::string g_create_err;
void ann_stream_release(annchor_ctx *c);
void ann_enemies_release(annchor_ctx *c);
void ann_draw_forget(annchor_ctx *c);   // features.hip
void ann_comm_release(annchor_ctx *c);
hipError_t ann_comm_guarded_sync(annchor_ctx *c, hipStream_t stream, const char *where);   // comm.hip

const char *ann_set_err(annchor_ctx *c, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    // (a collective's timeout is the cause of whatever HIP reports after the communicator's abort: keep saying so)
    if (c && c->comm_aborted && c->err.rfind("collective timed out", 0) == 0) return c->err.c_str();
    if (c) c->err = buf; else g_create_err = buf;
    return c ? c->err.c_str() : g_create_err.c_str();
}

// Large device allocations are kept for the next context instead of going back to the driver: a create / fit / close
// cycle at 127 M pairs allocates and frees ~10 buffers of 0.5-1 GB, and every fifth cycle or so one of those hipMalloc calls
// took 1.4 s on this stack (free memory constant; tools/repeat_fit.py) against 2 ms otherwise.  Blocks of 16 MB and more,
// at most pool_cap() bytes of them per process; a request takes the smallest cached block of its device that is large enough
// and not more than a quarter larger.  annchor_release_parked() returns them to the driver; ANNCHOR_NO_CTX_POOL=1 disables it.
namespace {
struct PoolBlock { void *p; size_t bytes; int device; };
std::mutex g_pool_mu;
std::vector<PoolBlock> g_pool;
size_t g_pool_bytes = 0;
constexpr size_t POOL_MIN_BLOCK = (size_t)16 << 20;
// the cap: half of the device's memory (144 GB here; ANNCHOR_CTX_POOL_GB overrides).  One context on a thinned list of 6 x 10^8
// pairs owns ~60 GB: with the first cap of 48 GB part of it went back to the driver at every close, and one fit in ten waited
// 4 s for its allocations (tools/lev100k_profile.py)
size_t pool_cap()
{
    static const size_t cap = [] {
        if (const char *e = getenv("ANNCHOR_CTX_POOL_GB")) return (size_t)atoll(e) << 30;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return (size_t)48 << 30; }
        return tot / 2;
    }();
    return cap;
}
bool pool_enabled()
{
    static const bool off = getenv("ANNCHOR_NO_CTX_POOL") != nullptr;
    return !off;
}
void *pool_take(int device, size_t want, size_t *got)
{
    if (want < POOL_MIN_BLOCK || !pool_enabled()) return nullptr;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    int best = -1;
    for (int i = 0; i < (int)g_pool.size(); ++i)
        if (g_pool[(size_t)i].device == device && g_pool[(size_t)i].bytes >= want && g_pool[(size_t)i].bytes <= want + want / 4 &&
            (best < 0 || g_pool[(size_t)i].bytes < g_pool[(size_t)best].bytes))
            best = i;
    if (best < 0) return nullptr;
    void *p = g_pool[(size_t)best].p;
    *got = g_pool[(size_t)best].bytes;
    g_pool_bytes -= *got;
    g_pool.erase(g_pool.begin() + best);
    return p;
}
}  // namespace
// hipMalloc through the pool (want rounded by the caller); *got = the block's real size
int ann_dev_alloc(annchor_ctx *c, void **p, size_t want, size_t *got)
{
    *got = want;
    static const bool trace_all = getenv("ANNCHOR_ALLOC_TRACE") && atoi(getenv("ANNCHOR_ALLOC_TRACE")) >= 2;
    if ((*p = pool_take(c->device, want, got)) != nullptr) {
        if (trace_all && want >= POOL_MIN_BLOCK) fprintf(stderr, "  pool hit  %9.1f MB -> block %9.1f MB (pool now %.1f GB)\n", (double)want / 1e6, (double)*got / 1e6, (double)g_pool_bytes / 1e9);
        return ANNCHOR_OK;
    }
    *got = want;
    if (trace_all && want >= POOL_MIN_BLOCK) fprintf(stderr, "  pool MISS %9.1f MB (pool now %.1f GB)\n", (double)want / 1e6, (double)g_pool_bytes / 1e9);
    if (hipMalloc(p, want) == hipSuccess) return ANNCHOR_OK;
    (void)hipGetLastError();
    *p = nullptr;
    {
        // out of memory with blocks parked in the pool: give them back to the driver and ask once more
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (PoolBlock &pb : g_pool) { (void)hipSetDevice(pb.device); (void)hipFree(pb.p); }
        g_pool.clear();
        g_pool_bytes = 0;
        (void)hipSetDevice(c->device);
    }
    ANN_CHECK_HIP(c, hipMalloc(p, want));
    return ANNCHOR_OK;
}

void ann_dev_free(annchor_ctx *c, void *p, size_t bytes)
{
    if (!p) return;
    if (bytes >= POOL_MIN_BLOCK && pool_enabled()) {
        // (the hipFree this replaces waited for the device: kernels queued on this context's stream may still read the block,
        // and the next taker may be another context with another stream)
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        // (an engine with a side stream: kernels of EITHER stream may still read the block, whichever one `stream` points at now)
        if (c->side_stream) {
            if (c->main_stream && c->main_stream != c->stream) (void)hipStreamSynchronize(c->main_stream);
            if (c->side_stream != c->stream) (void)hipStreamSynchronize(c->side_stream);
        }
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (g_pool_bytes + bytes <= pool_cap()) {
            g_pool.push_back({p, bytes, c->device});
            g_pool_bytes += bytes;
            static const bool trace_all = getenv("ANNCHOR_ALLOC_TRACE") && atoi(getenv("ANNCHOR_ALLOC_TRACE")) >= 2;
            if (trace_all) fprintf(stderr, "  to pool   %9.1f MB\n", (double)bytes / 1e6);
            return;
        }
    }
    (void)hipFree(p);
}

int ann_reserve(annchor_ctx *c, DevBuf &b, size_t bytes)
{
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return ANNCHOR_OK;
    size_t want = (bytes + 255) & ~(size_t)255;
    if (c->arena && c->arena_off + want <= c->arena_size) {
        if (b.p && !b.in_arena) ann_dev_free(c, b.p, b.cap);
        b.p = c->arena + c->arena_off;  // a previous (smaller) arena slice is simply abandoned
        c->arena_off += want;
        b.cap = want;
        b.in_arena = true;
        return ANNCHOR_OK;
    }
    static const bool trace = getenv("ANNCHOR_ALLOC_TRACE") != nullptr;   // stderr line per device allocation slower than 2 ms
    const auto t0 = std::chrono::steady_clock::now();
    if (b.p && !b.in_arena) ann_dev_free(c, b.p, b.cap);
    const auto t1 = std::chrono::steady_clock::now();
    b.p = nullptr;
    b.cap = 0;
    b.in_arena = false;
    size_t got = 0;
    ANN_TRY(ann_dev_alloc(c, &b.p, want, &got));
    want = got;
    b.cap = want;
    {
        // every member of the context that ever got an allocation of its own is released by annchor_destroy (a hand-kept list
        // there had fallen 18 buffers behind: ~1.3 GB leaked per context at 127 M pairs, and the device's allocator answered
        // the next contexts' gigabyte requests in 0.3-1.8 s instead of 2 ms)
        const char *lo = reinterpret_cast<const char *>(c), *me = reinterpret_cast<const char *>(&b);
        if (me >= lo && me < lo + sizeof(annchor_ctx) && std::find(c->own_allocs.begin(), c->own_allocs.end(), &b) == c->own_allocs.end())
            c->own_allocs.push_back(&b);
    }
    if (trace) {
        const double f = std::chrono::duration<double, std::milli>(t1 - t0).count();
        const double m = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        if (f + m > 2.0) fprintf(stderr, "alloc %.1f MB: free %.2f ms, malloc %.2f ms\n", (double)want / 1e6, f, m);
    }
    return ANNCHOR_OK;
}

int ann_arena_init(annchor_ctx *c, int64_t nx)
{
    // pair-list state is ~100 B per candidate pair (worst case: all pairs) + O(nx) rows
    double pairs = 0.5 * (double)nx * (double)(nx - 1);
    if (pairs > 32e6) pairs = 32e6;  // larger problems fall back to per-buffer allocations beyond the slab
    size_t bytes = (size_t)(pairs * 112.0) + (size_t)nx * 4096 + ((size_t)64 << 20);
    if (c->arena) {
        // one slab per context; a slab inherited from a parked context (see annchor_destroy) is kept
        // when it is large enough and nothing has been carved from it yet
        if (c->arena_size >= bytes || c->arena_off != 0) return ANNCHOR_OK;
        ann_dev_free(c, c->arena, c->arena_size);
        c->arena = nullptr;
        c->arena_size = 0;
    }
    void *p = nullptr;
    size_t got = 0;
    if ((p = pool_take(c->device, bytes, &got)) != nullptr) bytes = got;
    else if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return ANNCHOR_OK; }  // optional
    c->arena = (char *)p;
    c->arena_size = bytes;
    c->arena_off = 0;
    return ANNCHOR_OK;
}

// The small pieces of state the kernels expect to find ZERO the first time they run (sticky flags, the selection tables, the tie
// histogram, the classification cursors, the arrival slots of the persistent anchor launch): carved from the slab back to back
// when the data set is bound and cleared by ONE memset there, instead of six first-use memsets inside every first fit of a
// context (~5 us of host time each, most of them in front of a kernel the GPU is waiting for).  Without a slab (or once it is
// full) the first-use memsets remain.
int ann_prewarm_state(annchor_ctx *c)
{
    if (!c->arena || c->state_prewarmed) return ANNCHOR_OK;
    const size_t slot_bytes = sizeof(unsigned long long) * 4 * 1024 + 64;   // lev.hip: ann_lev_anchor_rounds
    struct Piece { DevBuf *b; size_t bytes; };
    Piece pieces[] = {{&c->dev_flags, sizeof(int32_t) * 16}, {&c->lev_cursors, 4 * sizeof(int32_t)}, {&c->sel_state, ann_sel_state_bytes()},
                      {&c->sel2, ann_sel2_table_bytes()},    {&c->tie_hist, ann_tie_hist_bytes()},   {&c->lev_ap, slot_bytes}};
    size_t need = 0;
    for (auto &q : pieces) {
        if (q.b->p) return ANNCHOR_OK;   // (already in use: leave everything to the first-use path)
        need += (q.bytes + 255) & ~(size_t)255;
    }
    if (c->arena_off + need > c->arena_size) return ANNCHOR_OK;
    char *first = c->arena + c->arena_off;
    for (auto &q : pieces) ANN_TRY(ann_reserve(c, *q.b, q.bytes));
    ANN_CHECK_HIP(c, hipMemsetAsync(first, 0, need, c->stream));
    c->dev_flags_clean = true;
    c->lev_cursor_epoch = 0;
    c->gn_err_clean = true;
    c->sel2_clean = c->sel2.p;
    c->tie_hist_clean = c->tie_hist.p;
    c->lev_ap_epoch = 0;
    c->state_prewarmed = true;
    return ANNCHOR_OK;
}

int ann_h2d(annchor_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return ANNCHOR_OK;
    if (c->pin && bytes <= annchor_ctx::PIN_SLOT_BYTES) {
        // small upload: copy into a pinned ring slot, enqueue, return -- the caller's buffer is
        // free again at once and the stream orders the copy before the kernels that follow
        const int sl = c->pin_next;
        c->pin_next = (sl + 1) % annchor_ctx::PIN_SLOTS;
        if (c->pin_busy[sl]) ANN_CHECK_HIP(c, hipEventSynchronize(c->pin_ev[sl]));
        unsigned char *slot = c->pin + (size_t)sl * annchor_ctx::PIN_SLOT_BYTES;
        memcpy(slot, src, bytes);
        ANN_CHECK_HIP(c, hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, c->stream));
        ANN_CHECK_HIP(c, hipEventRecord(c->pin_ev[sl], c->stream));
        c->pin_busy[sl] = true;
        return ANNCHOR_OK;
    }
    ANN_CHECK_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    ANN_CHECK_HIP(c, ann_sync(c, __func__));  // pageable host memory: do not retain the pointer
    return ANNCHOR_OK;
}

// Every host wait of the pair-list form goes through here: ANNCHOR_SYNC_TRACE=1 names them on stderr (tools/wait_census.py).
hipError_t ann_sync(annchor_ctx *c, const char *where)
{
    static const bool trace = getenv("ANNCHOR_SYNC_TRACE") != nullptr;
    static const bool timing = getenv("ANNCHOR_SYNC_TIMING") != nullptr;   // monotonic-clock stamps of every wait (tools/host_timeline.py)
    if (trace) fprintf(stderr, "sync %s\n", where);
    const long long t_in = timing ? ann_now_ns() : 0;
    if (c->idle_gen_n > c->idle_gen_done) {
        // host work parked for exactly this moment: the stream has just been given work and the caller is about to wait for it
        c->idle_gen_done = std::min(c->idle_gen_n, c->idle_gen_done + c->idle_gen_chunk);
        (void)ann_legacy_generate_upto(c->idle_gen_seed, c->idle_gen_n, c->idle_gen_done);
    }
    const long long t_w = timing ? ann_now_ns() : 0;
    if (c->side_pending) (void)ann_side_join(c);   // (a host wait covers the side stream's chains too)
    const hipError_t rc = c->comm ? ann_comm_guarded_sync(c, c->stream, where) : hipStreamSynchronize(c->stream);
    if (timing) fprintf(stderr, "T wait %s %lld %lld %lld\n", where, t_in, t_w, ann_now_ns());
    if (c->lev_ap_probe_epoch) ann_lev_ap_probe(c);
    return rc;
}

// The legacy sampler's MT19937 stream of `seed` (it depends on the seed only) produced on the calling thread at this context's NEXT
// host waits, `chunk` words per wait (<= 0: all at the first), i.e. after the caller has enqueued whatever it enqueues before it
// must wait: fit() parks the first draw's stream behind the anchor rounds -- annchor_build_locality's kernels are queued before the
// generation starts, and the second piece runs while the GPU emits the pair list and the features.
extern "C" int annchor_legacy_generate_at_next_wait(annchor_ctx *c, uint32_t seed, int64_t ndraws, int64_t chunk)
{
    if (!c || ndraws < 0) return ANNCHOR_EINVAL;
    c->idle_gen_seed = seed;
    c->idle_gen_n = ndraws;
    c->idle_gen_done = 0;
    c->idle_gen_chunk = chunk > 0 ? chunk : ndraws;
    return ANNCHOR_OK;
}

int ann_d2h(annchor_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return ANNCHOR_OK;
    if (c->pin && bytes <= annchor_ctx::PIN_DL_BYTES) {
        // (a pageable destination costs the runtime ~100 us of staging for a few hundred KB: the graph,
        // the sample's feature rows)
        unsigned char *slot = c->pin + (size_t)annchor_ctx::PIN_SLOTS * annchor_ctx::PIN_SLOT_BYTES;
        ANN_CHECK_HIP(c, hipMemcpyAsync(slot, src, bytes, hipMemcpyDeviceToHost, c->stream));
        ANN_CHECK_HIP(c, ann_sync(c, __func__));
        memcpy(dst, slot, bytes);
        return ANNCHOR_OK;
    }
    ANN_CHECK_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    ANN_CHECK_HIP(c, ann_sync(c, __func__));
    return ANNCHOR_OK;
}

// two small downloads, one wait
int ann_d2h2(annchor_ctx *c, void *dst1, const void *src1, size_t bytes1, void *dst2, const void *src2, size_t bytes2)
{
    const size_t off2 = (bytes1 + 63) & ~(size_t)63;
    if (c->pin && off2 + bytes2 <= annchor_ctx::PIN_DL_BYTES) {
        unsigned char *slot = c->pin + (size_t)annchor_ctx::PIN_SLOTS * annchor_ctx::PIN_SLOT_BYTES;
        ANN_CHECK_HIP(c, hipMemcpyAsync(slot, src1, bytes1, hipMemcpyDeviceToHost, c->stream));
        ANN_CHECK_HIP(c, hipMemcpyAsync(slot + off2, src2, bytes2, hipMemcpyDeviceToHost, c->stream));
        ANN_CHECK_HIP(c, ann_sync(c, __func__));
        memcpy(dst1, slot, bytes1);
        memcpy(dst2, slot + off2, bytes2);
        return ANNCHOR_OK;
    }
    ANN_TRY(ann_d2h(c, dst1, src1, bytes1));
    return ann_d2h(c, dst2, src2, bytes2);
}

// a small download the host waits for while MORE work is queued behind it: the copy goes to the pinned slot, an event marks
// its end, `then` enqueues what follows (it must not wait), the host waits for the event only
int ann_d2h_then(annchor_ctx *c, void *dst, const void *src, size_t bytes, int (*then)(annchor_ctx *))
{
    if (!c->pin || bytes > annchor_ctx::PIN_DL_BYTES) {
        ANN_TRY(ann_d2h(c, dst, src, bytes));
        return then(c);
    }
    if (!c->dl_ev) ANN_CHECK_HIP(c, hipEventCreate(&c->dl_ev));
    unsigned char *slot = c->pin + (size_t)annchor_ctx::PIN_SLOTS * annchor_ctx::PIN_SLOT_BYTES;
    ANN_CHECK_HIP(c, hipMemcpyAsync(slot, src, bytes, hipMemcpyDeviceToHost, c->stream));
    ANN_CHECK_HIP(c, hipEventRecord(c->dl_ev, c->stream));
    const int rc = then(c);
    static const bool trace = getenv("ANNCHOR_SYNC_TRACE") != nullptr;
    static const bool timing = getenv("ANNCHOR_SYNC_TIMING") != nullptr;
    if (trace) fprintf(stderr, "sync %s\n", __func__);
    const long long t_w = timing ? ann_now_ns() : 0;
    ANN_CHECK_HIP(c, hipEventSynchronize(c->dl_ev));
    if (timing) fprintf(stderr, "T wait %s %lld %lld %lld\n", __func__, t_w, t_w, ann_now_ns());
    memcpy(dst, slot, bytes);
    // (the probe's copy was queued before this download's: it has landed; a launch queued by `then` is a later one)
    return rc;
}

// ------------------------------------------------------------------ profiling
int ann_prof_entry(annchor_ctx *c, const char *name)
{
    for (size_t i = 0; i < c->prof.size(); ++i)
        if (c->prof[i].name == name || strcmp(c->prof[i].name, name) == 0) return (int)i;
    ProfEntry e;
    e.name = name;
    c->prof.push_back(e);
    return (int)c->prof.size() - 1;
}

static void prof_drain(annchor_ctx *c)
{
    for (auto &p : c->pending) {
        float ms = 0;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess)
            c->prof[p.entry].ms += ms;
        c->ev_pool.push_back(p.a);
        c->ev_pool.push_back(p.b);
    }
    c->pending.clear();
}

ProfScope::ProfScope(annchor_ctx *ctx, const char *name, double alg_bytes) : c(ctx)
{
    if (!c->prof_on) return;
    if (c->prof_mode == 2) {   // metric kernels only
        const size_t n = strlen(name);
        if (n < 6 || strcmp(name + n - 6, "_pairs") != 0) return;
    }
    entry = ann_prof_entry(c, name);
    c->prof[entry].launches += 1;
    c->prof[entry].alg_bytes += alg_bytes;
    if (entry == c->prof_group_entry) { entry = -1; return; }   // timed by the enclosing ProfGroup
    auto get = [&](hipEvent_t *e) {
        if (!c->ev_pool.empty()) { *e = c->ev_pool.back(); c->ev_pool.pop_back(); return true; }
        return hipEventCreate(e) == hipSuccess;
    };
    if (!get(&a) || !get(&b)) { entry = -1; return; }
    (void)hipEventRecord(a, c->stream);
}

ProfGroup::ProfGroup(annchor_ctx *ctx, const char *name) : c(ctx)
{
    if (!c->prof_on || c->prof_group_entry >= 0) return;
    if (c->prof_mode == 2) {   // metric kernels only
        const size_t n = strlen(name);
        if (n < 6 || strcmp(name + n - 6, "_pairs") != 0) return;
    }
    entry = ann_prof_entry(c, name);
    auto get = [&](hipEvent_t *e) {
        if (!c->ev_pool.empty()) { *e = c->ev_pool.back(); c->ev_pool.pop_back(); return true; }
        return hipEventCreate(e) == hipSuccess;
    };
    if (!get(&a) || !get(&b)) { entry = -1; return; }
    (void)hipEventRecord(a, c->stream);
    c->prof_group_entry = entry;
}

ProfGroup::~ProfGroup()
{
    if (entry < 0) return;
    (void)hipEventRecord(b, c->stream);
    c->pending.push_back({entry, a, b});
    c->prof_group_entry = -1;
}

ProfScope::~ProfScope()
{
    if (entry < 0) return;
    (void)hipEventRecord(b, c->stream);
    c->pending.push_back({entry, a, b});
    if (c->pending.size() > 4096) prof_drain(c);
}

extern "C" int annchor_prof_enable(annchor_ctx *c, int32_t on)
{
    if (!c) return ANNCHOR_EINVAL;
    c->prof_on = on != 0;
    c->prof_mode = on;
    return ANNCHOR_OK;
}

extern "C" int annchor_prof_reset(annchor_ctx *c)
{
    if (!c) return ANNCHOR_EINVAL;
    prof_drain(c);
    for (auto &e : c->prof) { e.ms = 0; e.launches = 0; e.alg_bytes = 0; }
    return ANNCHOR_OK;
}

extern "C" int annchor_prof_get(annchor_ctx *c, int32_t max_entries, const char **names, double *ms,
                                int64_t *launches, double *alg_bytes)
{
    if (!c) return ANNCHOR_EINVAL;
    (void)ann_sync(c, __func__);
    prof_drain(c);
    int n = 0;
    for (auto &e : c->prof) {
        if (n >= max_entries) break;
        names[n] = e.name;
        ms[n] = e.ms;
        launches[n] = e.launches;
        alg_bytes[n] = e.alg_bytes;
        ++n;
    }
    return n;
}

// ------------------------------------------------------------------ lifecycle
// What a context needs from the runtime besides its buffers.  A destroyed context parks these for
// the next one on the same device: hipStreamCreate / hipStreamDestroy / hipHostMalloc / hipHostFree
// and the slab's hipMalloc / hipFree add up to ~4 ms per context on this stack
// (tools/lifecycle_time.py), against a 5.5 ms fit.  Parked shells are never freed (process exit).
struct CtxShell {
    int device = 0;
    hipDeviceProp_t prop;
    hipStream_t stream = nullptr, side_stream = nullptr;
    hipEvent_t side_fork_ev = nullptr, side_done_ev = nullptr, trace_ev = nullptr;
    unsigned char *pin = nullptr;
    hipEvent_t pin_ev[annchor_ctx::PIN_SLOTS] = {};
    hipEvent_t call_a = nullptr, call_b = nullptr;
    std::vector<hipEvent_t> ev_pool;
    char *arena = nullptr;
    size_t arena_size = 0;
};
static std::mutex g_shell_mu;
static std::vector<CtxShell> g_shells;
static constexpr size_t SHELL_MAX = 4;
static constexpr size_t SHELL_ARENA_MAX = (size_t)2 << 30;

// The engine's side stream (fit() overlap).  ANNCHOR_FIT_OVERLAP is read HERE, per engine: 0 keeps every kernel on the
// engine's one stream in the order of the staged calls.  The side stream is created right behind the engine's own where the
// engine creates both: in the traces taken so far two streams created back to back sat on different hardware queues (observed
// behaviour of the runtime, not a documented guarantee; an engine that takes over a parked shell without a side stream creates
// its own later, and nothing is known about that pair).
static int side_init(annchor_ctx *c)
{
    c->main_stream = c->stream;
    const char *e = getenv("ANNCHOR_FIT_OVERLAP");
    c->overlap_parts = (e && atoi(e) == 0) ? 0 : 1;
    if (!c->overlap_parts || c->side_stream) return ANNCHOR_OK;
    if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->side_fork_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->side_done_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->trace_ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        c->overlap_parts = 0;   // (no second stream to be had: everything stays on the engine's own)
    }
    return ANNCHOR_OK;
}

int ann_side_fork(annchor_ctx *c)
{
    ANN_CHECK_HIP(c, hipEventRecord(c->side_fork_ev, c->main_stream));
    ANN_CHECK_HIP(c, hipStreamWaitEvent(c->side_stream, c->side_fork_ev, 0));
    return ANNCHOR_OK;
}

int ann_side_join(annchor_ctx *c)
{
    if (!c->side_pending) return ANNCHOR_OK;
    c->side_pending = false;
    ANN_CHECK_HIP(c, hipStreamWaitEvent(c->main_stream, c->side_done_ev, 0));
    return ANNCHOR_OK;
}

SideScope::SideScope(annchor_ctx *ctx) : c(ctx) { c->stream = c->side_stream; }
SideScope::~SideScope()
{
    (void)hipEventRecord(c->side_done_ev, c->side_stream);
    c->side_pending = true;
    c->stream = c->main_stream;
}

// What the overlap did, for tests: out[0] = 1 when the engine has a side stream in use, out[1] = the calls of
// annchor_update_bounds that found their computed-neighbour lists prepared.  Reads host state only.
extern "C" int annchor_overlap_stats(annchor_ctx *c, int64_t *out)
{
    if (!c || !out) return ANNCHOR_EINVAL;
    out[0] = c->overlap_parts != 0 && c->side_stream != nullptr;
    out[1] = c->ub_prepared_taken;
    return ANNCHOR_OK;
}

extern "C" int annchor_create(int device, annchor_ctx **out)
{
    if (!out) return ANNCHOR_EINVAL;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        ann_set_err(nullptr, "no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return ANNCHOR_ENODEV;
    }
    if (device < 0 || device >= count) {
        ann_set_err(nullptr, "device %d out of range (have %d)", device, count);
        return ANNCHOR_EINVAL;
    }
    annchor_ctx *c = new annchor_ctx();
    c->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess) {
        ann_set_err(nullptr, "device init failed: %s", hipGetErrorString(e));
        delete c;
        return ANNCHOR_EHIP;
    }
    {
        // a parked shell of this device (stream, pinned staging, events, device slab): creating and
        // destroying those costs ~4 ms per context, more than half a C2 fit
        std::lock_guard<std::mutex> lk(g_shell_mu);
        for (size_t i = 0; i < g_shells.size(); ++i)
            if (g_shells[i].device == device) {
                CtxShell &sh = g_shells[i];
                c->prop = sh.prop; c->stream = sh.stream; c->pin = sh.pin;
                c->side_stream = sh.side_stream; c->side_fork_ev = sh.side_fork_ev; c->side_done_ev = sh.side_done_ev; c->trace_ev = sh.trace_ev;
                for (int k = 0; k < annchor_ctx::PIN_SLOTS; ++k) c->pin_ev[k] = sh.pin_ev[k];
                c->call_a = sh.call_a; c->call_b = sh.call_b;
                c->ev_pool.swap(sh.ev_pool);
                c->arena = sh.arena; c->arena_size = sh.arena_size; c->arena_off = 0;
                g_shells.erase(g_shells.begin() + (long)i);
                *out = c;
                return side_init(c);
            }
    }
    if ((e = hipGetDeviceProperties(&c->prop, device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        ann_set_err(nullptr, "device init failed: %s", hipGetErrorString(e));
        delete c;
        return ANNCHOR_EHIP;
    }
    (void)hipEventCreate(&c->call_a);
    (void)hipEventCreate(&c->call_b);
    if (getenv("ANNCHOR_NO_PIN") ||
        hipHostMalloc((void **)&c->pin, annchor_ctx::PIN_SLOTS * annchor_ctx::PIN_SLOT_BYTES + annchor_ctx::PIN_DL_BYTES + annchor_ctx::PIN_TAIL_BYTES, hipHostMallocDefault) != hipSuccess)
        c->pin = nullptr;   // fall back to pageable transfers
    for (int i = 0; i < annchor_ctx::PIN_SLOTS; ++i) (void)hipEventCreateWithFlags(&c->pin_ev[i], hipEventDisableTiming);
    *out = c;
    return side_init(c);
}

extern "C" void annchor_destroy(annchor_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)ann_sync(c, __func__);
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);   // (nothing of this engine is in flight when its streams are parked or destroyed)
    ann_draw_forget(c);
    prof_drain(c);
    ann_comm_release(c);
    ann_stream_release(c);
    ann_enemies_release(c);
    for (DevBuf *b : c->own_allocs)
        if (b->p && !b->in_arena) { ann_dev_free(c, b->p, b->cap); b->p = nullptr; b->cap = 0; }
    c->own_allocs.clear();
    if (c->dl_ev) { c->ev_pool.push_back(c->dl_ev); c->dl_ev = nullptr; }
    {
        // park the shell for the next context of this device (at most SHELL_MAX of them, slabs up to
        // SHELL_ARENA_MAX; ANNCHOR_NO_CTX_POOL=1 turns the parking off)
        static const bool no_pool = getenv("ANNCHOR_NO_CTX_POOL") != nullptr;
        std::lock_guard<std::mutex> lk(g_shell_mu);
        if (!no_pool && g_shells.size() < SHELL_MAX && c->stream && c->pin) {
            CtxShell sh;
            sh.device = c->device; sh.prop = c->prop; sh.stream = c->stream; sh.pin = c->pin;
            for (int k = 0; k < annchor_ctx::PIN_SLOTS; ++k) sh.pin_ev[k] = c->pin_ev[k];
            sh.call_a = c->call_a; sh.call_b = c->call_b;
            sh.side_stream = c->side_stream; sh.side_fork_ev = c->side_fork_ev; sh.side_done_ev = c->side_done_ev; sh.trace_ev = c->trace_ev;
            sh.ev_pool.swap(c->ev_pool);
            sh.arena = c->arena; sh.arena_size = c->arena_size;
            if (sh.arena && sh.arena_size > SHELL_ARENA_MAX) { ann_dev_free(c, sh.arena, sh.arena_size); sh.arena = nullptr; sh.arena_size = 0; }
            g_shells.push_back(std::move(sh));
            delete c;
            return;
        }
    }
    if (c->arena) ann_dev_free(c, c->arena, c->arena_size);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < annchor_ctx::PIN_SLOTS; ++i)
        if (c->pin_ev[i]) (void)hipEventDestroy(c->pin_ev[i]);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->call_a) (void)hipEventDestroy(c->call_a);
    if (c->call_b) (void)hipEventDestroy(c->call_b);
    if (c->side_fork_ev) (void)hipEventDestroy(c->side_fork_ev);
    if (c->side_done_ev) (void)hipEventDestroy(c->side_done_ev);
    if (c->trace_ev) (void)hipEventDestroy(c->trace_ev);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

// free the parked context shells (device slabs, pinned staging, streams); contexts in use are untouched
extern "C" int annchor_parked_bytes(int device, int64_t *bytes)
{
    if (!bytes) return ANNCHOR_EINVAL;
    size_t tot = 0;
    {
        std::lock_guard<std::mutex> lk(g_shell_mu);
        for (const CtxShell &sh : g_shells) if (sh.device == device && sh.arena) tot += sh.arena_size;
    }
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (const PoolBlock &pb : g_pool) if (pb.device == device) tot += pb.bytes;
    }
    *bytes = (int64_t)tot;
    return ANNCHOR_OK;
}

extern "C" int annchor_release_parked(void)
{
    std::vector<CtxShell> shells;
    {
        std::lock_guard<std::mutex> lk(g_shell_mu);
        shells.swap(g_shells);
    }
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (PoolBlock &pb : g_pool) { (void)hipSetDevice(pb.device); (void)hipFree(pb.p); }
        g_pool.clear();
        g_pool_bytes = 0;
    }
    for (CtxShell &sh : shells) {
        (void)hipSetDevice(sh.device);
        if (sh.arena) (void)hipFree(sh.arena);
        for (hipEvent_t e : sh.ev_pool) (void)hipEventDestroy(e);
        for (int i = 0; i < annchor_ctx::PIN_SLOTS; ++i)
            if (sh.pin_ev[i]) (void)hipEventDestroy(sh.pin_ev[i]);
        if (sh.pin) (void)hipHostFree(sh.pin);
        if (sh.call_a) (void)hipEventDestroy(sh.call_a);
        if (sh.call_b) (void)hipEventDestroy(sh.call_b);
        if (sh.side_fork_ev) (void)hipEventDestroy(sh.side_fork_ev);
        if (sh.side_done_ev) (void)hipEventDestroy(sh.side_done_ev);
        if (sh.trace_ev) (void)hipEventDestroy(sh.trace_ev);
        if (sh.side_stream) (void)hipStreamDestroy(sh.side_stream);
        if (sh.stream) (void)hipStreamDestroy(sh.stream);
    }
    return (int)shells.size();
}

// PCI bus id of a device ("0000:c1:00.0"): lets a launcher bind its process to the CPUs of the
// GPU's NUMA node (/sys/bus/pci/devices/<id>/numa_node) before it creates contexts
extern "C" int annchor_device_pci_bus_id(int device, char *buf, int buflen)
{
    if (!buf || buflen < 16) return ANNCHOR_EINVAL;
    return hipDeviceGetPCIBusId(buf, buflen, device) == hipSuccess ? ANNCHOR_OK : ANNCHOR_EHIP;
}

// free / total device memory in bytes (the host sizes the pair-list form from it: ~130 B per candidate pair)
extern "C" int annchor_device_mem_info(int device, int64_t *free_bytes, int64_t *total_bytes)
{
    if (!free_bytes || !total_bytes) return ANNCHOR_EINVAL;
    size_t f = 0, t = 0;
    if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&f, &t) != hipSuccess) { (void)hipGetLastError(); return ANNCHOR_EHIP; }
    *free_bytes = (int64_t)f;
    *total_bytes = (int64_t)t;
    return ANNCHOR_OK;
}

extern "C" const char *annchor_last_error(annchor_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }
extern "C" const char *annchor_create_error(void) { return g_create_err.c_str(); }

extern "C" int annchor_device_name(annchor_ctx *c, char *buf, int buflen)
{
    if (!c || !buf || buflen <= 0) return ANNCHOR_EINVAL;
    snprintf(buf, (size_t)buflen, "%s (%s, %d CUs)", c->prop.name, c->prop.gcnArchName, c->prop.multiProcessorCount);
    return ANNCHOR_OK;
}

extern "C" int annchor_synchronize(annchor_ctx *c)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_CHECK_HIP(c, ann_sync(c, __func__));
    return ANNCHOR_OK;
}

extern "C" int annchor_last_kernel_ms(annchor_ctx *c, float *ms)
{
    if (!c || !ms) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, c->call_timed, ANNCHOR_EINVAL, "no timed call yet");
    ANN_CHECK_HIP(c, hipEventSynchronize(c->call_b));
    ANN_CHECK_HIP(c, hipEventElapsedTime(ms, c->call_a, c->call_b));
    return ANNCHOR_OK;
}
