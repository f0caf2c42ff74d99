// pmx_api.hip - the host half of libpmx.so: the C ABI of include/pmx.h over the kernels of pmx_screen.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <cstddef>
#include <memory>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include <time.h>

#include "pmx.h"
#include "pmx_screen.hip"
#include "pmx_handles.h"
#include "pmx_debug.h"
#include "pmx_explain.h"
#include "pmx_rows.h"
#include "pmx_model_tables.h"

using namespace pmx;

// -------------------------------------------------------------------------------------- state
static thread_local pmx_score_stats g_stats = {};
static int g_profiling = 0;
struct ScreenWs;
static thread_local std::shared_ptr<ScreenWs> g_last_screen;
static thread_local int g_last_device = 0;
static int screen_stats(pmx_score_stats *out);

int pmx_profiling() { return g_profiling; }

extern "C" int pmx_set_profiling(int enabled) {
    g_profiling = enabled;
    return PMX_OK;
}
extern "C" int pmx_score_stats_get(pmx_score_stats *out) {
    if (!out) return pmx_fail(PMX_ERR_INVALID, "null stats");
    *out = g_stats;
    if (g_last_screen) return screen_stats(out);
    return PMX_OK;
}

// -------------------------------------------------------------------------------------- model
static_assert(sizeof(F2) == sizeof(float2) && offsetof(F2, y) == offsetof(float2, y), "F2 is float2");
static_assert(sizeof(F4) == sizeof(float4) && offsetof(F4, y) == offsetof(float4, y) && offsetof(F4, z) == offsetof(float4, z) && offsetof(F4, w) == offsetof(float4, w),
              "F4 is float4");
static_assert(sizeof(FnCell) == kFnCellBytes, "the size limit of build_model_tables");

// Cells whose polynomial deviates from the function by more than this, relative to the function, are flagged (FnCell) and
// evaluated term by term where a self entry meets them. 2e-7 is just above what the float32 coefficients themselves cost
// (each rounded to 6e-8 of its value) and leaves room for the reference's own float32 rounding of z and z^2 (about
// 1e-7 z^2 / 2 relative) within the 2e-6 the parity tests allow; on the bench library 1-3 self items per ligand are flagged.
static double fn_rel_tol() {
    const char *s = std::getenv("PMX_FN_RELTOL");
    const double v = (s && *s) ? std::atof(s) : 2e-7;
    return v > 0.0 ? v : 2e-7;
}

// ... and cells where the terms that make up the function are beyond exp(-8) of their peaks (weighted mean of z^2 / 2 above 8,
// |z| > 4): there the reference's own float32 rounding of z and z^2 reaches 1.4e-6 of the value, and only the same operations
// in the same order reproduce it. ([MI355X] round 6: 6 -> 8. A flagged lane makes its whole wavefront walk the term-by-term loop: 6.8 -> 3.1 flagged self values
// per ligand on the bench library, 92.6 -> 91.0 ms per pass, every score of the 10^6 ligands the same bits; the tail sweeps of tests/test_gpu_tails.py and
// test_gpu_pair_tails.py hold at their 2e-6 - 1.8e-6 against the term-by-term engine - and fail narrowly, 1.87e-6, at 9.)
static double fn_max_exponent() {
    const char *s = std::getenv("PMX_FN_MAXEXP");
    const double v = (s && *s) ? std::atof(s) : 8.0;
    return v > 0.0 ? v : 8.0;
}

// The tabulated functions for the call's weights: built on `stream` the first time, kept for the last four weight sets.
static int pair_functions(pmx_model *m, const Weights &W, hipStream_t stream, FnTable *out) {
    std::lock_guard<std::mutex> lock(m->fn_mu);
    FnEntry *hit = nullptr;
    for (FnEntry &e : m->fn)
        if (std::memcmp(&e.W, &W, sizeof(W)) == 0) hit = &e;
    if (!hit) {
        if (m->fn.size() < 4) {
            FnEntry fresh; // (enters the cache only once its buffer and event exist)
            PMX_HIPCHECK(hipMalloc((void **)&fresh.cells, (size_t)m->NF * m->ncell * sizeof(FnCell)));
            const hipError_t ee = hipEventCreateWithFlags(&fresh.ready, hipEventDisableTiming);
            if (ee != hipSuccess) {
                (void)hipFree(fresh.cells);
                return pmx_fail(PMX_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(ee));
            }
            m->fn.push_back(fresh);
            hit = &m->fn.back();
        } else { // recycle the least recently used entry once nothing queued still reads it
            hit = &m->fn[0];
            for (FnEntry &e : m->fn)
                if (e.stamp < hit->stamp) hit = &e;
            PMX_HIPCHECK(hipDeviceSynchronize());
        }
        hit->W = W;
        fn_build_kernel<<<dim3(m->NF), dim3(128), 0, stream>>>(m->dm, W, m->sub_off, m->sub_nodes, m->NS, m->ncell, m->h, m->win, hit->cells, fn_rel_tol(), fn_max_exponent());
        PMX_HIPCHECK(hipGetLastError());
        PMX_HIPCHECK(hipEventRecord(hit->ready, stream));
    } else {
        PMX_HIPCHECK(hipStreamWaitEvent(stream, hit->ready, 0));
    }
    hit->stamp = ++m->fn_stamp;
    out->cells = hit->cells;
    out->plane16 = m->NF * m->ncell;
    out->NS = m->NS;
    out->tri = m->dm.symmetric != 0 ? 1u : 0u;
    out->ncell = m->ncell;
    out->inv_h = 1.0f / m->h;
    return PMX_OK;
}

// The model's tables (build_model_tables), uploaded: one allocation of 16-byte aligned sections, one copy.
extern "C" int pmx_model_create(const pmx_model_desc *d, int device, pmx_model **out) {
    if (!d || !out) return pmx_fail(PMX_ERR_INVALID, "null argument");
    ModelTables t;
    const int rc = build_model_tables(d, &t);
    if (rc != PMX_OK) return rc;
    PMX_HIPCHECK(hipSetDevice(device));

    std::vector<unsigned char> host;
    auto section = [&host](const auto &v) { // appends a table, returns its offset
        const size_t off = host.size(), bytes = v.size() * sizeof(v[0]);
        host.resize(off + round16(bytes), 0);
        if (bytes) std::memcpy(host.data() + off, v.data(), bytes);
        return off;
    };
    const size_t off_edge = section(t.edge), off_type = section(t.node_type), off_tclus = section(t.tclus), off_cpair = section(t.cpair), off_cwin = section(t.cwin);
    const size_t off_sidtab = section(t.sidtab), off_sub_off = section(t.sub_off), off_sub_nodes = section(t.sub_nodes), off_win = section(t.win);
    host.resize(host.size() + 16, 0);

    void *blob = nullptr;
    PMX_HIPCHECK(hipMalloc(&blob, host.size()));
    const hipError_t e = hipMemcpy(blob, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(blob);
        return pmx_fail(PMX_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(e));
    }
    const unsigned char *b8 = static_cast<const unsigned char *>(blob);
    pmx_model *m = new pmx_model();
    m->device = device;
    m->blob = blob;
    std::memcpy(m->node_type, t.node_type.data(), sizeof(m->node_type));
    m->dm.Nm = t.Nm;
    m->dm.K = t.K;
    m->dm.symmetric = t.symmetric;
    m->dm.pad_ = 0;
    m->dm.edge = reinterpret_cast<const float4 *>(b8 + off_edge);
    m->dm.node_type = b8 + off_type;
    m->dm.tclus = reinterpret_cast<const uint64_t *>(b8 + off_tclus);
    m->dm.cpair = reinterpret_cast<const float2 *>(b8 + off_cpair);
    m->dm.cwin = reinterpret_cast<const float2 *>(b8 + off_cwin);
    m->NS = t.NS;
    m->NF = t.NF;
    m->ncell = t.ncell;
    m->h = t.h;
    m->sidtab = reinterpret_cast<const uint16_t *>(b8 + off_sidtab);
    m->sub_off = reinterpret_cast<const uint32_t *>(b8 + off_sub_off);
    m->sub_nodes = b8 + off_sub_nodes;
    m->win = reinterpret_cast<const float2 *>(b8 + off_win);
    *out = m;
    return PMX_OK;
}

extern "C" int pmx_model_destroy(pmx_model *m) {
    if (!m) return PMX_OK;
    (void)hipSetDevice(m->device);
    (void)hipFree(m->blob);
    for (FnEntry &e : m->fn) {
        if (e.cells) (void)hipFree(e.cells);
        if (e.ready) (void)hipEventDestroy(e.ready);
    }
    delete m;
    return PMX_OK;
}

// ------------------------------------------------------------------------------------ library
extern "C" int pmx_library_upload(const pmx_library_view *v, int device, pmx_library **out) {
    if (!v || !out) return pmx_fail(PMX_ERR_INVALID, "null argument");
    if (!v->offsets) return pmx_fail(PMX_ERR_INVALID, "null offsets");
    PMX_HIPCHECK(hipSetDevice(device));
    const uint64_t n = v->n_ligands;
    const hipMemcpyKind kind = v->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    uint64_t nbytes = 0;
    if (v->on_device) {
        PMX_HIPCHECK(hipMemcpy(&nbytes, v->offsets + n, 8, hipMemcpyDeviceToHost));
    } else {
        nbytes = v->offsets[n];
    }
    const bool adopt = v->on_device == 2;
    if (adopt && !v->data) return pmx_fail(PMX_ERR_INVALID, "null data");
    pmx_library *lib = new pmx_library();
    lib->device = device;
    lib->offsets = nullptr;
    lib->data = nullptr;
    lib->owns = !adopt;
    hipError_t e = hipSuccess;
    if (adopt) { // the buffers stay the caller's: no allocation, no copy
        lib->offsets = const_cast<uint64_t *>(v->offsets);
        lib->data = const_cast<uint8_t *>(v->data);
    } else {
        e = hipMalloc((void **)&lib->offsets, (n + 1) * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&lib->data, std::max<uint64_t>(nbytes, 16));
        if (e == hipSuccess) e = hipMemcpy(lib->offsets, v->offsets, (n + 1) * 8, kind);
        if (e == hipSuccess && nbytes) e = hipMemcpy(lib->data, v->data, nbytes, kind);
    }
    // The counters live in one small buffer per device that is never freed: hipFree waits for every stream of the device, and an adopted
    // library is made while other streams copy and score ([MI355X] the pipeline's scoring calls each started when the NEXT chunk's copy had ended).
    static std::mutex stats_mu;
    static unsigned long long *stats_of_device[64] = {};
    unsigned long long stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    lib->dl.n = n;
    lib->dl.offsets = lib->offsets;
    lib->dl.data = lib->data;
    if (e == hipSuccess && (device < 0 || device >= 64)) e = hipErrorInvalidDevice;
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lock(stats_mu);
        unsigned long long *&stats_dev = stats_of_device[device];
        if (!stats_dev) e = hipMalloc((void **)&stats_dev, sizeof(stats));
        if (e == hipSuccess) e = hipMemset(stats_dev, 0, sizeof(stats));
        if (e == hipSuccess && n) {
            library_stats_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(lib->dl, lib->data, nbytes, stats_dev);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(stats, stats_dev, sizeof(stats), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) {
        if (lib->owns && lib->offsets) (void)hipFree(lib->offsets);
        if (lib->owns && lib->data) (void)hipFree(lib->data);
        delete lib;
        return pmx_fail(e == hipErrorOutOfMemory ? PMX_ERR_OOM : PMX_ERR_HIP, "library upload failed: %s", hipGetErrorString(e));
    }
    if (stats[5]) { // offsets are validated on the device, for host and device views alike
        if (lib->owns) (void)hipFree(lib->offsets), (void)hipFree(lib->data);
        delete lib;
        return pmx_fail(PMX_ERR_INVALID, "%llu record offsets are not 16-byte aligned, run backwards or point past the data", stats[5]);
    }
    lib->info.n_ligands = n;
    lib->info.n_bytes = nbytes;
    lib->info.total_conformers = stats[0];
    lib->info.max_nodes = (int32_t)stats[1];
    lib->info.max_conformers = (int32_t)stats[2];
    lib->info.max_clusters = (int32_t)stats[3];
    lib->info.n_unsupported = (int32_t)stats[4];
    *out = lib;
    return PMX_OK;
}

extern "C" int pmx_library_info_get(const pmx_library *lib, pmx_library_info *info) {
    if (!lib || !info) return pmx_fail(PMX_ERR_INVALID, "null argument");
    *info = lib->info;
    return PMX_OK;
}

extern "C" int pmx_library_buffers(const pmx_library *lib, const uint64_t **offsets_dev, const uint8_t **data_dev) {
    if (!lib || !offsets_dev || !data_dev) return pmx_fail(PMX_ERR_INVALID, "null argument");
    *offsets_dev = lib->offsets;
    *data_dev = lib->data;
    return PMX_OK;
}

extern "C" int pmx_library_destroy(pmx_library *lib) {
    if (!lib) return PMX_OK;
    (void)hipSetDevice(lib->device);
    if (lib->owns) (void)hipFree(lib->offsets), (void)hipFree(lib->data);
    delete lib;
    return PMX_OK;
}

// ---------------------------------------------------------------------------------- helpers
static std::mutex g_mu;

static long env_long(const char *name, long dflt) {
    const char *s = std::getenv(name);
    if (!s || !*s) return dflt;
    return std::atol(s);
}

static constexpr size_t kLdsPerCu = 160 * 1024;

static bool trace_on() {
    static int v = -1;
    if (v < 0) v = std::getenv("PMX_TRACE") ? 1 : 0;
    return v == 1;
}

// ------------------------------------------------------------------------------------ the screening engine (pmx_screen.hip)
// A call is cut into chunks of <= PMX_SUPER ligands (per pocket); a chunk is: clear the control block; ligand_kernel over the
// range (tables in per-wave slices); ligand_kernel over the ligands whose tables need larger slices / the arena; a fixed
// number of task rounds (each a snapshot of the queue + one persistent launch that exits at once when the round is empty; the
// last round never queues); finalize; the arena retries. Everything goes out on the caller's stream, in order: a chunk is
// through with the control block, arena, queue and lists when the next one starts, so a workspace holds one of each. Nothing
// is read back, no host thread.
struct ScreenWs {
    DevBuf ctl;                      // Ctl: pmx_score's control block
    DevBuf xctl;                     // Ctl: pmx_explain's (its own: the statistics of the last pmx_score stay what that call left)
    DevBuf slices, big;              // per-wavefront table slices, large slices
    DevBuf totbuf;                   // ligand kernel's wavefronts | task kernel's
    DevBuf pabuf;                    // path_bound()'s pair sums: ligand kernel's wavefronts | task kernel's
    DevBuf arena, queue;
    DevBuf lists;                    // uint32: ovf | carry | heavy
    DevBuf acur;                     // uint32: the row cursor of pmx_attribute and pmx_align
    size_t arena_shrunk_to = 0;      // the arena size that was accepted when memory was short (0: never shrunk)
    int num_cu = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // profiling: call start | last chunk: ligand kernels start, done | end | last chunk: rounds start, done
    uint64_t ligands_last = 0;
    bool ev_valid = false;
    bool ctl_used = false; // the call in progress has cleared `ctl`
    hipStream_t last_stream = nullptr;
    std::mutex mu; // held while a call enqueues (the workspace belongs to one call at a time, in stream order)
    uint64_t stamp = 0;    // last use (ensure_screen): the least recently used workspace of a device goes first
    bool released = false; // pmx_release_workspaces (or the cap on workspaces per device) took the buffers: a caller that was waiting on `mu` asks for a new workspace
    void free_buffers() {
        for (DevBuf *b : {&ctl, &xctl, &slices, &big, &totbuf, &pabuf, &arena, &queue, &lists, &acur}) b->release();
        for (auto &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        arena_shrunk_to = 0;
        ev_valid = ctl_used = false;
    }
};
// Workspaces are shared: the map, a call in progress and the thread that asks for the last call's statistics each hold a
// reference, so pmx_release_workspaces can take a workspace out of the map and free its buffers while none of them is left
// with a dangling pointer (the object itself goes with its last reference).
static std::map<std::pair<int, hipStream_t>, std::shared_ptr<ScreenWs>> g_screen; // (device, stream)

static uint64_t g_screen_stamp = 0;

// The workspace of (device, stream), made on first use. At most PMX_MAX_WORKSPACES (default 4) are kept per device: a host
// program that scores on short-lived streams would otherwise leave some 40 GB behind per stream it ever used (the key is the raw
// stream handle; nothing tells libpmx that a stream is gone). When one more is needed the least recently used idle one is
// taken out of the map and freed - after a device synchronisation, its stream may no longer exist - and a caller that was
// waiting for it finds it `released` and asks again.
static std::shared_ptr<ScreenWs> ensure_screen(int device, hipStream_t stream) {
    std::shared_ptr<ScreenWs> out, victim;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        const auto key = std::make_pair(device, stream);
        auto it = g_screen.find(key);
        if (it != g_screen.end() && it->second) {
            it->second->stamp = ++g_screen_stamp;
            return it->second;
        }
        const long cap = std::max<long>(1, env_long("PMX_MAX_WORKSPACES", 4));
        long have = 0;
        for (const auto &kv : g_screen) have += kv.first.first == device && kv.second ? 1 : 0;
        if (have >= cap) {
            auto lru = g_screen.end();
            for (auto jt = g_screen.begin(); jt != g_screen.end(); ++jt) {
                if (jt->first.first != device || !jt->second) continue;
                if (lru != g_screen.end() && jt->second->stamp >= lru->second->stamp) continue;
                if (!jt->second->mu.try_lock()) continue; // a call is enqueuing on it
                if (lru != g_screen.end()) lru->second->mu.unlock();
                lru = jt;
            }
            if (lru != g_screen.end()) {
                victim = std::move(lru->second); // (its mutex is held)
                g_screen.erase(lru);
            }
        }
        out = std::make_shared<ScreenWs>();
        out->stamp = ++g_screen_stamp;
        g_screen[key] = out;
    }
    if (victim) {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        victim->free_buffers();
        victim->released = true;
        victim->mu.unlock();
    }
    return out;
}

// The per-wavefront buffers of a workspace, in bytes (a call grows them to the largest need of its pockets).
struct BufferNeeds {
    size_t slices = 0, big = 0, totbuf = 0, pabuf = 0;
    void cover(const BufferNeeds &o) { slices = std::max(slices, o.slices), big = std::max(big, o.big), totbuf = std::max(totbuf, o.totbuf), pabuf = std::max(pabuf, o.pabuf); }
};

static int grow_buffers(ScreenWs &ws, const BufferNeeds &need, hipStream_t stream) {
    PMX_HIPCHECK(ws.slices.grow(need.slices, stream));
    PMX_HIPCHECK(ws.big.grow(need.big, stream));
    PMX_HIPCHECK(ws.totbuf.grow(need.totbuf, stream));
    PMX_HIPCHECK(ws.pabuf.grow(need.pabuf, stream));
    return PMX_OK;
}

// The table arena of a workspace. (A smaller arena than asked for with PMX_ARENA_MB is slower - more trees walked by one
// wavefront alone - never wrong, so it shrinks when memory is short: several streams each keep a workspace. A size that was
// accepted after shrinking stands until the workspace is released: asking for the full size again on every call would
// synchronise, free and fail again each time)
// (32 / 64 conformer lanes: records of megabytes - 16 GB held the split trees of a 16 384-ligand chunk of the stress configuration
// to within 3 %, and every tree past the end is walked by one wavefront alone)
// ([MI355X] round 6: 64 GB at up to 16 lanes. SURVEY 8d-2's library puts 29 GB of split trees' tables into the arena per 1 M-ligand chunk at the old
// budget, 17 GB at the new one; with a 16 GB arena 200 000 trees found it full and were walked by one wavefront each - the longest for 1.2 M
// passes, the pass 3.4 s instead of 0.54 s. The part has 288 GB.)
template <int G>
static int ensure_arena(ScreenWs &ws, hipStream_t stream) {
    size_t arena_want = (size_t)std::max<long>(1, env_long("PMX_ARENA_MB", G >= 32 ? 32768 : 65536)) << 20;
    if (!ws.arena.ptr && !std::getenv("PMX_ARENA_MB")) { // first allocation, no explicit size: at most a third of what the device has free
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b / 3 < arena_want) {
            arena_want = std::max<size_t>((size_t)1 << 30, (free_b / 3) & ~(((size_t)1 << 20) - 1));
            ws.arena_shrunk_to = arena_want;
        } else {
            (void)hipGetLastError();
        }
    }
    const size_t arena_min = std::min<size_t>((size_t)1 << 30, arena_want);
    if (ws.arena_shrunk_to) arena_want = std::min(arena_want, std::max(ws.arena_shrunk_to, arena_min));
    PMX_HIPCHECK(ws.arena.grow(arena_want, stream, arena_min));
    if (ws.arena.bytes < arena_want) ws.arena_shrunk_to = ws.arena.bytes;
    return PMX_OK;
}

// Arena pass t + 2 (mode 3) over the ligands the arena pass before had no room for: it reads the list that pass wrote and lists
// what it has no room for in the other half of `lists` - the last one lists nothing, it reports them.
static void prepare_retry(ScreenParams &p, Ctl *ctl, uint32_t *lists, uint32_t cap, int t, int retries, hipStream_t stream) {
    retry_prep_kernel<<<dim3(1), dim3(64), 0, stream>>>(ctl, (uint32_t)(t + 1) & 1u);
    p.retry_in = (t & 1) == 0 ? lists : lists + cap;
    p.retry_out = t + 1 == retries ? nullptr : ((t & 1) == 0 ? lists + cap : lists);
    p.retry_slot = (uint32_t)(t + 1) & 1u;
}

// Events and control block of a workspace, on its first call (num_cu is set last: a workspace whose events or control block
// could not be made stays uninitialised).
static int init_workspace(ScreenWs &ws, int device, hipStream_t stream) {
    if (ws.num_cu) return PMX_OK;
    auto init = [&]() -> int {
        hipDeviceProp_t prop;
        PMX_HIPCHECK(hipGetDeviceProperties(&prop, device));
        for (auto &e : ws.ev) PMX_HIPCHECK(hipEventCreate(&e));
        PMX_HIPCHECK(ws.ctl.grow(sizeof(Ctl), stream));
        ws.num_cu = prop.multiProcessorCount;
        return PMX_OK;
    };
    const int irc = init();
    if (irc) ws.free_buffers();
    return irc;
}

// Type weights further apart than PMX_TAILS_RATIO (default 8 = the ratio of the reference's own defaults, graph_match.py:32-40: any override that spreads the weights further takes the exact tails): pair items
// evaluate rough cells term by term like self items do (item_finish<TAILS>, pmx_screen_tables.h) - slower, and only then.
// PMX_PAIR_TAILS = 0 / 1 forces it off / on. Decided per pocket, by the types it holds: pmx_score_multi scores each pocket as pmx_score scores
// it alone and as pmx_explain explains it, whatever else is in the panel (tests/test_gpu_library_select.py).
static bool pair_tails(const pmx_model *model, const Weights &W) {
    float wmin = INFINITY, wmax = 0.f;
    bool present[PMX_NUM_TYPES] = {};
    for (int i = 0; i < model->dm.Nm; ++i) present[model->node_type[i]] = true; // (only the types the pocket holds can meet in an entry)
    for (int t = 0; t < PMX_NUM_TYPES; ++t) {
        const float a = std::fabs(W.w[t]);
        if (present[t] && a > 0.f && std::isfinite(a)) wmin = std::min(wmin, a), wmax = std::max(wmax, a);
    }
    const char *rs = std::getenv("PMX_TAILS_RATIO");
    const double ratio = (rs && *rs) ? std::atof(rs) : 8.0;
    bool tails = wmax > 0.f && (double)wmax > ratio * (double)wmin;
    const long force = env_long("PMX_PAIR_TAILS", -1);
    if (force == 0) tails = false;
    if (force > 0) tails = true;
    return tails;
}

// What one pocket of a call needs: kernel parameters, launch shapes, buffers and chunk size. pmx_score and pmx_explain both plan
// here: the same workspace serves both, and explain promises the score pass's slices, large slices, arena passes and statuses.
// `p` holds what the model and the library decide; what one call decides (flags, range, budget, outputs, lists, control block)
// its caller sets.
struct PocketPlan {
    ScreenParams p;
    size_t lds = 0;
    uint32_t waves_per_cu = 0, task_waves_per_cu = 0;
    uint32_t slice_bytes = 0, big_bytes = 0, big_grid = 0;
    uint32_t super = 0;
    int arena_retries = 0; // arena passes after the first (0: no table of this model and library can exceed a large slice)
    BufferNeeds need;
};

template <int G>
static int plan_pocket(const pmx_model *model, const pmx_library *lib, const Weights &W, int num_cu, hipStream_t stream, PocketPlan &pl) {
    pl = PocketPlan{};
    ScreenParams &p = pl.p;
    p.M = model->dm;
    const int rc = pair_functions(const_cast<pmx_model *>(model), W, stream, &p.F);
    if (rc) return rc;
    p.lib = lib->dl;
    p.sidtab = model->sidtab;
    p.sub_off = model->sub_off;
    p.sub_nodes = model->sub_nodes;
    p.W = W;
    p.max_nodes = (uint32_t)std::max(4, std::min(lib->info.max_nodes, PMX_MAX_LIGAND_NODES));
    p.bound_cost = (uint32_t)std::max<long>(0, env_long("PMX_BOUND_COST", 8192));
    p.dead_min_entries = (uint32_t)std::max<long>(1, env_long("PMX_DEAD_MIN_ENTRIES", 32));
    const WaveShape<G> shape = wave_shape<G>(model->dm.K, (int)p.max_nodes);
    pl.lds = shape.bytes;
    pl.waves_per_cu = (uint32_t)std::max<long>(2, std::min<long>({(long)(kLdsPerCu / shape.bytes), 4L * PMX_SCREEN_WAVES, env_long("PMX_WAVES_PER_CU", 32)}));
    // the task kernel is the walker alone: it may be built for more waves per SIMD than the ligand kernel (PMX_TASK_WAVES)
    pl.task_waves_per_cu = (uint32_t)std::max<long>(2, std::min<long>({(long)(kLdsPerCu / shape.bytes), 4L * PMX_TASK_WAVES, env_long("PMX_TASK_WAVES_PER_CU", 32)}));
    const uint32_t grid = (uint32_t)num_cu * std::max(pl.waves_per_cu, pl.task_waves_per_cu); // (sizes the per-wavefront buffers of both kernels)
    // per-wavefront slice: 112 KB at 8 conformer lanes (every ligand of the bench library fits, path_bound()'s table included), scaled with the lanes
    // (table bytes grow with the square of the model's cluster count: the 11-cluster 6OIM-like model is the reference point)
    const long k_scale = std::max(1L, std::min(16L, ((long)model->dm.K * model->dm.K + 60) / 121));
    pl.slice_bytes = (uint32_t)std::max<long>(4, env_long("PMX_SLICE_KB", (cand_bounds<G>() ? 112L : 80L) * std::max(1, G / 8) * k_scale)) * 1024u;
    pl.need.slices = (size_t)grid * pl.slice_bytes;
    // large slices for the ligands whose tables exceed a slice: as large as a table of this model and library can get, at most
    // PMX_BIG_SLICE_MB each, PMX_BIG_TOTAL_MB together (what is larger still goes to the arena)
    const uint64_t nlmax = (uint64_t)std::min<int>(PMX_MAX_LEVELS, std::max(1, lib->info.max_clusters));
    const uint64_t K = (uint64_t)std::max(1, std::min(model->dm.K, PMX_MAX_LEVEL_CANDIDATES)); // (candidates per level)
    const uint64_t worst = rec_bytes<G>((uint32_t)(nlmax * K), (uint32_t)(nlmax * (nlmax - 1) / 2 * K * K), (uint32_t)nlmax);
    const uint64_t cap = (uint64_t)std::max<long>(1, env_long("PMX_BIG_SLICE_MB", G >= 32 ? 4 : 32)) << 20;
    pl.big_bytes = (uint32_t)std::max<uint64_t>(pl.slice_bytes, (std::min(worst, cap) + 4095) & ~4095ull);
    const uint64_t total = (uint64_t)std::max<long>(64, env_long("PMX_BIG_TOTAL_MB", G >= 32 ? 16384 : 4096)) << 20;
    pl.big_grid = (uint32_t)std::max<uint64_t>(16, std::min<uint64_t>(grid, total / pl.big_bytes));
    pl.need.big = (size_t)pl.big_grid * pl.big_bytes;
    if (cand_bounds<G>()) { // float[matches <= levels][candidates of all levels][G], at most 1 MB per wavefront (larger jobs do without)
        const uint64_t need = (nlmax + 1) * nlmax * K * G * 4;
        p.pa_bytes = (uint32_t)std::min<uint64_t>((need + 255) & ~255ull, (uint64_t)std::max<long>(1, env_long("PMX_PATH_KB", 1024)) << 10);
        pl.need.pabuf = (size_t)grid * p.pa_bytes * 2u; // ligand kernel | task kernel
    }
    // (the table phase stages node distances and chain lengths there at 32 / 64 lanes)
    if (!totals_in_lds<G>()) pl.need.totbuf = (size_t)num_cu * 4u * std::max(PMX_SCREEN_WAVES, PMX_TASK_WAVES) * kTotBufBytes * 2u; // ligand kernel | task kernel
    // arena passes over the ligands an arena pass had no room for, each with the arena to itself (a pass with an empty list exits at
    // once): a ligand is reported PMX_LIGAND_TOO_LARGE when its tables exceed the whole arena - or when the arena-class ligands of a
    // chunk need more than 1 + PMX_ARENA_RETRIES arenas
    if (worst > pl.big_bytes) pl.arena_retries = (int)std::max<long>(1, env_long("PMX_ARENA_RETRIES", 4));
    // chunk: what the arena has to hold at a time are the tables of the chunk's split trees. (Cutting a pocket's pass into more
    // chunks than the arena asks for does not pay: every chunk ends in a dozen rounds with a tail each - 1 M ligands in 8
    // chunks: 258 ms, 207 ms in one chunk.)
    const long super_dflt = std::max(16384L, (1L << 20) * 8 / std::max(G, 8) / k_scale);
    pl.super = (uint32_t)std::max<long>(1024, std::min<long>(env_long("PMX_SUPER", super_dflt), 1 << 24));
    return PMX_OK;
}

// The table passes of one chunk, in the one order pmx_score and pmx_explain both run them: every ligand whose tables fit a slice; the
// others with large slices (fewer wavefronts); what exceeds those from the arena - ligands that find it full (of the tables of over-budget
// trees, or of each other) are listed in the storage of the overflow list, which is done with; then those, with the arena to themselves
// (only models and libraries whose largest tables exceed a large slice have such passes), the last pass reporting what still does not
// fit. launch(mode, blocks) starts the caller's kernel on `p`; grid0 is the slice pass's grid, `grid` every later pass's. after_pass()
// runs behind every arena pass and says whether to go on (PMX_OK).
template <class Launch, class AfterPass>
static int chunk_passes(ScreenParams &p, const PocketPlan &pl, const ScreenWs &ws, uint32_t grid0, uint32_t grid, hipStream_t stream, Launch launch, AfterPass after_pass) {
    p.slices = ws.slices.as<uint8_t>();
    p.slice_bytes = pl.slice_bytes;
    launch(0, grid0);
    p.slices = ws.big.as<uint8_t>();
    p.slice_bytes = pl.big_bytes;
    launch(1, grid);
    p.retry_out = p.ovf_list;
    p.retry_slot = 0;
    launch(2, grid);
    int rc = after_pass();
    for (int t = 0; t < pl.arena_retries && !rc; ++t) {
        prepare_retry(p, p.ctl, p.ovf_list, p.list_cap, t, pl.arena_retries, stream);
        launch(3, grid);
        rc = after_pass();
    }
    p.retry_in = nullptr;
    return rc;
}

template <int G>
static int score_screen(const pmx_model *const *models, int n_models, const pmx_library *lib, const Weights &W, uint64_t first, uint64_t count,
                        void *scores_dev, bool scores_f64, int32_t *status_dev, hipStream_t stream, ScreenWs &ws) {
    if (count > 0xfffffff0ull) return pmx_fail(PMX_ERR_INVALID, "more than 2^32 ligands in one call");
    // ---- knobs
    const uint32_t flags = (uint32_t)env_long("PMX_TREE_FLAGS", 0);
    // [MI355X] round 6, passes a walk may take before it splits. On the bench library (92 passes per ligand, 7 % of the walks over 384) 384 / 384
    // and 768 / 384 are the same 99.1 ms; on SURVEY 8d-2's own library (800 passes per ligand) 384 sends 57-74 % of the ligands to the arena and
    // the queue (714 ms with a 64 GB arena, queue full), 768 a third of them (539 ms). A queued subtree keeps the smaller budget: the rounds' tail.
    const uint32_t lig_budget = (uint32_t)std::max<long>(16, env_long("PMX_BUDGET", 768));
    const uint32_t task_budget = (uint32_t)std::max<long>(16, env_long("PMX_TASK_BUDGET", std::min<long>(lig_budget, 384))); // a queued subtree's own budget
    const int rounds = (int)std::max<long>(1, env_long("PMX_ROUNDS", 12));
    const int task_decay_from = (int)std::max<long>(1, env_long("PMX_TASK_DECAY_FROM", 99));
    const uint32_t task_budget_min = (uint32_t)std::max<long>(8, env_long("PMX_TASK_BUDGET_MIN", 48));
    const bool exact = (flags & 8) != 0;
    // any validation switch: the kernels of pmx_screen_debug.hip (libpmx's own read those bits as zero, pmx_screen_layout.h PMX_WFLAGS)
    const bool debug_kernels = (flags & ~PMX_PRODUCT_FLAGS) != 0;

    // ---- plan: per pocket, parameters and launch shapes
    {
        const int irc = init_workspace(ws, lib->device, stream);
        if (irc) return irc;
    }
    std::vector<PocketPlan> plan((size_t)n_models);
    BufferNeeds need;
    uint32_t super_max = 0;
    for (int m = 0; m < n_models; ++m) {
        PocketPlan &pl = plan[(size_t)m];
        const int rc = plan_pocket<G>(models[m], lib, W, ws.num_cu, stream, pl);
        if (rc) return rc;
        ScreenParams &p = pl.p;
        p.first = first;
        p.flags = flags | (scores_f64 ? PMX_SCORES_F64 : 0u);
        p.budget = lig_budget;
        p.min_levels = (uint32_t)std::max<long>(0, env_long("PMX_MIN_LEVELS", 3));
        p.scores = scores_f64 ? reinterpret_cast<float *>(static_cast<double *>(scores_dev) + (size_t)m * count) : static_cast<float *>(scores_dev) + (size_t)m * count;
        p.status = m == 0 ? status_dev : nullptr;
        need.cover(pl.need);
        super_max = std::max(super_max, pl.super);
    }

    // ---- buffers
    {
        int rc = grow_buffers(ws, need, stream);
        if (!rc) rc = ensure_arena<G>(ws, stream);
        if (rc) return rc;
        PMX_HIPCHECK(ws.queue.grow((size_t)std::max<long>(1, env_long("PMX_TASKQ_MB", (G >= 32 ? 1024L : 2048L) * std::max(1, G / 8))) << 20, stream));
        PMX_HIPCHECK(ws.lists.grow((size_t)super_max * 12, stream));
    }
    Ctl *const ctl = ws.ctl.as<Ctl>();
    uint32_t *const lists = ws.lists.as<uint32_t>();
    uint8_t *const totbuf = ws.totbuf.as<uint8_t>(), *const pabuf = ws.pabuf.as<uint8_t>();

    // ---- pockets and their chunks
    if (g_profiling) PMX_HIPCHECK(hipEventRecord(ws.ev[0], stream));
    ws.ctl_used = false;
    for (int m = 0; m < n_models; ++m) {
        const PocketPlan &pl = plan[(size_t)m];
        ScreenParams p = pl.p;
        const bool tails = pair_tails(models[m], W); // (term-by-term tails for widely spread type weights, see pair_tails)
        const uint32_t super = pl.super;
        const uint32_t lig_grid = (uint32_t)ws.num_cu * pl.waves_per_cu, task_grid = (uint32_t)ws.num_cu * pl.task_waves_per_cu;
        p.ctl = ctl;
        p.arena = ws.arena.as<uint8_t>();
        p.arena_bytes = std::min<unsigned long long>(ws.arena.bytes, (1ull << 36) - 4096);
        p.ovf_list = lists;
        p.carry_list = lists + super;
        p.heavy_list = lists + 2 * (size_t)super;
        p.list_cap = super;
        p.queue = ws.queue.as<uint8_t>();
        p.qcap = (uint32_t)std::min<size_t>(ws.queue.bytes / task_rec_bytes<G>() / kShards, 0x3fffffffu / kShards);
        p.totbuf = totbuf; // (the ligand kernel's halves; rounds_and_finalize switches to the task kernel's and back)
        p.pabuf = pabuf;
        auto launch = [&](int mode, uint32_t blocks) {
            p.mode = mode;
            if (debug_kernels) pmx_debug::launch_ligand(G, exact, tails, blocks, pl.lds, stream, p);
            else if (tails) ligand_kernel<G, false, true><<<dim3(blocks), dim3(64), pl.lds, stream>>>(p);
            else ligand_kernel<G, false, false><<<dim3(blocks), dim3(64), pl.lds, stream>>>(p);
        };
        // the subtrees the over-budget walkers queued, and the ones those queue in turn: a fixed number of rounds, each a snapshot of
        // the queue and one persistent launch (an empty round exits at once); the last round walks everything to its end
        auto rounds_and_finalize = [&]() {
            if (!totals_in_lds<G>()) p.totbuf = totbuf + ws.totbuf.bytes / 2;
            if (pabuf) p.pabuf = pabuf + ws.pabuf.bytes / 2;
            for (int r = 0; r < rounds; ++r) {
                // Late rounds hold few subtrees (fewer than wavefronts): what they cost is their longest walk, i.e. the budget. Halving
                // it from round PMX_TASK_DECAY_FROM on spreads a deep subtree over the idle wavefronts sooner.
                p.budget = r < task_decay_from ? task_budget : std::max<uint32_t>(task_budget_min, task_budget >> std::min(r - task_decay_from + 1, 16));
                p.last_round = r + 1 == rounds ? 1u : 0u;
                round_kernel<<<dim3(1), dim3(64), 0, stream>>>(ctl, p.qcap);
                if (debug_kernels) pmx_debug::launch_task(G, task_grid, pl.lds, stream, p);
                else task_kernel<G><<<dim3(task_grid), dim3(64), pl.lds, stream>>>(p);
            }
            finalize_kernel<G><<<dim3((super + 255) / 256), dim3(256), 0, stream>>>(p);
            p.last_round = 0;
            p.budget = lig_budget;
            p.totbuf = totbuf;
            p.pabuf = pabuf;
        };
        for (uint64_t lo = 0; lo < count; lo += super) {
            const bool last_of_call = m + 1 == n_models && lo + super >= count;
            p.lo = (uint32_t)lo;
            p.hi = (uint32_t)std::min<uint64_t>(count, lo + super);
            if (g_profiling && last_of_call) PMX_HIPCHECK(hipEventRecord(ws.ev[1], stream));
            ws.ligands_last = p.hi - p.lo;
            ctl_clear_kernel<<<dim3((sizeof(Ctl) / 4 + 255) / 256), dim3(256), 0, stream>>>(ctl, ws.ctl_used ? 0 : 1);
            ws.ctl_used = true;
            bool mark = g_profiling && last_of_call; // the first arena pass of the call's last chunk ends the ligand kernels and starts the rounds
            const int rc = chunk_passes(p, pl, ws, lig_grid, std::min(pl.big_grid, lig_grid), stream, launch, [&]() -> int {
                if (mark) {
                    PMX_HIPCHECK(hipEventRecord(ws.ev[2], stream));
                    PMX_HIPCHECK(hipEventRecord(ws.ev[4], stream));
                    mark = false;
                }
                rounds_and_finalize();
                return PMX_OK;
            });
            if (rc) return rc;
            if (g_profiling && last_of_call) PMX_HIPCHECK(hipEventRecord(ws.ev[5], stream));
        }
    }
    PMX_HIPCHECK(hipGetLastError());
    if (g_profiling) PMX_HIPCHECK(hipEventRecord(ws.ev[3], stream));
    ws.ev_valid = g_profiling != 0;
    ws.last_stream = stream;
    return PMX_OK;
}

// Statistics of the last call on this thread's workspace: synchronises the stream the call ran on.
static int screen_stats(pmx_score_stats *out) {
    const std::shared_ptr<ScreenWs> w = g_last_screen;
    if (!w) return PMX_OK;
    std::lock_guard<std::mutex> lock(w->mu);
    if (w->released || !w->num_cu) return PMX_OK; // (the workspace was released after the call: its counters went with it)
    PMX_HIPCHECK(hipSetDevice(g_last_device));
    PMX_HIPCHECK(hipStreamSynchronize(w->last_stream));
    unsigned long long st[kStatWords] = {0};
    std::vector<unsigned char> host(sizeof(Ctl));
    *out = pmx_score_stats{};
    if (w->ctl_used) {
        PMX_HIPCHECK(hipMemcpy(host.data(), w->ctl.ptr, sizeof(Ctl), hipMemcpyDeviceToHost));
        const Ctl *c = reinterpret_cast<const Ctl *>(host.data());
        for (int sh = 0; sh < kScreenStatShards; ++sh)
            for (int i = 0; i < kStatWords; ++i) st[i] = (i == 5) ? std::max(st[i], c->stats[sh][i]) : st[i] + c->stats[sh][i];
        out->queue_overflow = c->qflag;
        out->arena_bytes = c->arena_top;
        out->arena_capacity = w->arena.bytes;
    }
    out->n_frames = st[0];
    out->n_passes = st[1];
    out->n_heavy = st[2];
    out->n_items = st[3];
    out->n_exact_cells = st[4];
    out->max_passes = st[5];
    out->n_tasks = st[6];
    out->n_slice_overflow = st[7] & 0xffffffffull;
    out->n_probes = st[7] >> 32;
    out->n_probe_passes = st[15];
    out->n_exported = st[14];
    out->n_exact_values = st[13];
    for (int i = 0; i < 6; ++i) out->dbg[i] = st[16 + i];
    out->n_path_bounds = st[22];
    out->n_path_drops = st[23];
    out->n_dead_entries = st[24];
    out->ticks_scan = st[8], out->ticks_tables = st[9], out->ticks_bounds = st[10], out->ticks_walk = st[11], out->ticks_alive = st[12];
    out->ligands_last = w->ligands_last;
    if (w->ev_valid) {
        float ms = 0.f;
        PMX_HIPCHECK(hipEventElapsedTime(&ms, w->ev[0], w->ev[3]));
        out->ms_total = ms;
        PMX_HIPCHECK(hipEventElapsedTime(&ms, w->ev[1], w->ev[2]));
        out->ms_ligand = ms;
        PMX_HIPCHECK(hipEventElapsedTime(&ms, w->ev[4], w->ev[5]));
        out->ms_tasks = ms;
    }
    return PMX_OK;
}

// Conformer lanes per slot for a library: its most conformers, rounded up to a power of two.
static int lanes_of(const pmx_library *lib) {
    int g = 1;
    while (g < std::min(lib->info.max_conformers, PMX_MAX_CONFORMERS)) g <<= 1;
    return g;
}

// The workspace of (device, stream), held: one call at a time enqueues on it. (lock is released before ws goes)
struct HeldWs {
    std::shared_ptr<ScreenWs> ws;
    std::unique_lock<std::mutex> lock;
};
static HeldWs hold_screen(int device, hipStream_t stream) {
    for (;;) {
        HeldWs h{ensure_screen(device, stream), {}};
        h.lock = std::unique_lock<std::mutex>(h.ws->mu);
        if (!h.ws->released) return h; // (released while this call waited: the map holds a fresh one, or will make one)
    }
}

static int score_any(const pmx_model *const *models, int n_models, const pmx_library *lib, const float weights[PMX_NUM_TYPES], uint64_t first,
                     uint64_t count, void *scores_dev, bool scores_f64, int32_t *status_dev, void *stream_) {
    if (!models || n_models < 0 || !lib || !weights || (!scores_dev && count && n_models)) return pmx_fail(PMX_ERR_INVALID, "null argument");
    for (int i = 0; i < n_models; ++i) {
        if (!models[i]) return pmx_fail(PMX_ERR_INVALID, "null model");
        if (models[i]->device != lib->device) return pmx_fail(PMX_ERR_INVALID, "model and library live on different devices");
    }
    if (first > lib->info.n_ligands || count > lib->info.n_ligands - first) return pmx_fail(PMX_ERR_INVALID, "ligand range out of bounds");
    g_stats = pmx_score_stats{};
    g_last_screen.reset();
    if (count == 0 || n_models == 0) return PMX_OK;
    PMX_HIPCHECK(hipSetDevice(lib->device));
    const Weights W = to_weights(weights);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const HeldWs held = hold_screen(lib->device, stream);
    int rc = PMX_OK;
    if (!with_lanes(lanes_of(lib), [&](auto g) { rc = score_screen<decltype(g)::value>(models, n_models, lib, W, first, count, scores_dev, scores_f64, status_dev, stream, *held.ws); }))
        rc = pmx_fail(PMX_ERR_INVALID, "no kernels for %d conformer lanes", lanes_of(lib));
    g_last_screen = held.ws;
    g_last_device = lib->device;
    return rc;
}

extern "C" int pmx_score_multi(const pmx_model *const *models, int n_models, const pmx_library *lib,
                               const float weights[PMX_NUM_TYPES], uint64_t first, uint64_t count, float *scores_dev,
                               int32_t *status_dev, void *stream) {
    return score_any(models, n_models, lib, weights, first, count, scores_dev, false, status_dev, stream);
}

extern "C" int pmx_score(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], uint64_t first,
                         uint64_t count, float *scores_dev, int32_t *status_dev, void *stream) {
    if (!model) return pmx_fail(PMX_ERR_INVALID, "null argument");
    return score_any(&model, 1, lib, weights, first, count, scores_dev, false, status_dev, stream);
}

// The same with the score as the float64 the reference returns (graph_match.py:109: `float(np.mean(...))` of float64 maxima).
extern "C" int pmx_score_multi_f64(const pmx_model *const *models, int n_models, const pmx_library *lib,
                                   const float weights[PMX_NUM_TYPES], uint64_t first, uint64_t count, double *scores_dev,
                                   int32_t *status_dev, void *stream) {
    return score_any(models, n_models, lib, weights, first, count, scores_dev, true, status_dev, stream);
}

extern "C" int pmx_score_f64(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], uint64_t first,
                             uint64_t count, double *scores_dev, int32_t *status_dev, void *stream) {
    if (!model) return pmx_fail(PMX_ERR_INVALID, "null argument");
    return score_any(&model, 1, lib, weights, first, count, scores_dev, true, status_dev, stream);
}


// Frees the cached scoring workspaces of `device` (table arenas, task queues, class lists, fused-engine buffers): they are
// grown on demand and kept between calls, which is what a screening loop wants and what a long-lived host program that
// is done screening does not.
extern "C" int pmx_release_workspaces(int device) {
    PMX_HIPCHECK(hipSetDevice(device));
    PMX_HIPCHECK(hipDeviceSynchronize());
    std::vector<std::shared_ptr<ScreenWs>> taken;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        for (auto it = g_screen.begin(); it != g_screen.end();) {
            if (it->first.first != device) {
                ++it;
                continue;
            }
            taken.push_back(std::move(it->second));
            it = g_screen.erase(it);
        }
    }
    for (auto &w : taken) {
        std::lock_guard<std::mutex> wl(w->mu); // a call that is enqueuing on this workspace finishes first
        PMX_HIPCHECK(hipDeviceSynchronize());       // ... and what it enqueued
        w->free_buffers();
        w->released = true;
    }
    int rc = pmx_topk_release(device);
    if (!rc) rc = pmx_pack_release(device);
    if (!rc) rc = pmx_select_release(device);
    return rc ? rc : pmx_enrich_release(device);
}

// ------------------------------------------------------------------------------------ explain (pmx_explain.hip)
// The listed ligands' tables are built as pmx_score builds them - per-wave slices, then large slices, then the arena with its
// retries - and each is walked to its end by one wavefront of the explain kernel: no budget, no task queue.
template <int G>
static int explain_screen(const pmx_model *model, const pmx_library *lib, const Weights &W, const pmx_xpl::Args &a, bool constrained, hipStream_t stream,
                          ScreenWs &ws) {
    int rc = init_workspace(ws, lib->device, stream);
    if (rc) return rc;
    const bool tails = pair_tails(model, W); // (as pmx_score, pmx_score_multi and their _f64 forms decide it for this model)
    PocketPlan pl;
    rc = plan_pocket<G>(model, lib, W, ws.num_cu, stream, pl);
    if (!rc) rc = grow_buffers(ws, pl.need, stream);
    if (!rc && !ws.arena.ptr) rc = ensure_arena<G>(ws, stream); // (an arena made by pmx_score is taken as it is)
    if (rc) return rc;
    PMX_HIPCHECK(ws.lists.grow((size_t)a.n * 12, stream));
    PMX_HIPCHECK(ws.xctl.grow(sizeof(Ctl), stream));
    Ctl *const xctl = ws.xctl.as<Ctl>();
    uint32_t *const lists = ws.lists.as<uint32_t>();
    ScreenParams &p = pl.p;
    p.flags = PMX_SCORES_F64; // (never PMX_TREE_FLAGS)
    p.status = a.status;
    p.ctl = xctl;
    p.arena = ws.arena.as<uint8_t>();
    p.arena_bytes = std::min<unsigned long long>(ws.arena.bytes, (1ull << 36) - 4096);
    p.ovf_list = lists;
    p.carry_list = lists + a.n;
    p.heavy_list = lists + 2 * (size_t)a.n;
    p.list_cap = a.n;
    p.pabuf = ws.pabuf.as<uint8_t>();
    p.totbuf = ws.totbuf.as<uint8_t>();
    p.hi = a.n;

    pmx_xpl::launch_init(a, stream);
    ctl_clear_kernel<<<dim3((sizeof(Ctl) / 4 + 255) / 256), dim3(256), 0, stream>>>(xctl, 1);
    const size_t lds = pmx_xpl::lds_bytes(G, model->dm.K, (int)p.max_nodes, constrained, (int)a.n_modes);
    const uint32_t full = (uint32_t)ws.num_cu * pl.waves_per_cu;
    auto launch = [&](int mode, uint32_t blocks) {
        p.mode = mode;
        pmx_xpl::launch(G, tails, constrained, std::max(1u, blocks), (unsigned)lds, stream, p, a);
    };
    (void)chunk_passes(p, pl, ws, std::min(full, a.n), std::min(pl.big_grid, full), stream, launch, [] { return PMX_OK; }); // (no rounds: every walk ends in its pass)
    pmx_xpl::launch_fixup(a, stream);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}

// pmx_explain, pmx_explain_constrained and pmx_explain_modes: one driver; without a constraint the kernels are the ones that never look at
// one. n_modes leaves per conformer, 1 for pmx_explain and pmx_explain_constrained: the outputs are [n][n_modes][...].
static int explain_call(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const pmx_match_constraint *constraint,
                        int n_modes, const uint64_t *ligands_dev, uint32_t n, double *conf_max_dev, uint8_t *match_dev, uint8_t *levels_dev, int32_t *best_conformer_dev,
                        int32_t *status_dev, void *stream_) {
    if (!model || !lib || !weights) return pmx_fail(PMX_ERR_INVALID, "null argument");
    pmx_match_constraint con;
    std::memset(&con, 0, sizeof con);
    if (constraint) {
        const int K = model->dm.K;
        const auto beyond = [K](const uint64_t w[2]) { // a bit at or above the model's cluster count
            const uint64_t m0 = K >= 64 ? ~0ull : (1ull << K) - 1ull, m1 = K >= 128 ? ~0ull : (K > 64 ? (1ull << (K - 64)) - 1ull : 0ull);
            return ((w[0] & ~m0) | (w[1] & ~m1)) != 0ull;
        };
        if (constraint->n_require < 0 || constraint->n_require > PMX_MAX_REQUIRE_GROUPS)
            return pmx_fail(PMX_ERR_INVALID, "constraint: %d require groups (0 to %d)", (int)constraint->n_require, PMX_MAX_REQUIRE_GROUPS);
        con.n_require = constraint->n_require;
        for (int g = 0; g < con.n_require; ++g) {
            if ((constraint->require[g][0] | constraint->require[g][1]) == 0ull) return pmx_fail(PMX_ERR_INVALID, "constraint: require group %d is empty", g);
            if (beyond(constraint->require[g])) return pmx_fail(PMX_ERR_INVALID, "constraint: require group %d names a cluster outside the model's %d", g, K);
            con.require[g][0] = constraint->require[g][0];
            con.require[g][1] = constraint->require[g][1];
        }
        if (beyond(constraint->exclude)) return pmx_fail(PMX_ERR_INVALID, "constraint: the exclude set names a cluster outside the model's %d", K);
        con.exclude[0] = constraint->exclude[0];
        con.exclude[1] = constraint->exclude[1];
    }
    if (n > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "more than %d ligands in one explain call", PMX_EXPLAIN_MAX);
    if ((uint64_t)n * (uint64_t)n_modes > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "%u ligands x %d modes: more than %d in one call", n, n_modes, PMX_EXPLAIN_MAX);
    if (n == 0) return PMX_OK;
    if (!ligands_dev || !conf_max_dev || !match_dev || !levels_dev || !best_conformer_dev || !status_dev) return pmx_fail(PMX_ERR_INVALID, "null argument");
    if (model->device != lib->device) return pmx_fail(PMX_ERR_INVALID, "model and library live on different devices");
    PMX_HIPCHECK(hipSetDevice(lib->device));
    const Weights W = to_weights(weights);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const pmx_xpl::Args a{ligands_dev, n, (uint32_t)n_modes, conf_max_dev, match_dev, levels_dev, best_conformer_dev, status_dev, con};
    const bool constrained = constraint != nullptr;
    const HeldWs held = hold_screen(lib->device, stream);
    int rc = PMX_OK;
    if (!with_lanes(lanes_of(lib), [&](auto g) { rc = explain_screen<decltype(g)::value>(model, lib, W, a, constrained, stream, *held.ws); }))
        rc = pmx_fail(PMX_ERR_INVALID, "no kernels for %d conformer lanes", lanes_of(lib));
    return rc;
}

extern "C" int pmx_explain(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const uint64_t *ligands_dev, uint32_t n,
                           double *conf_max_dev, uint8_t *match_dev, uint8_t *levels_dev, int32_t *best_conformer_dev, int32_t *status_dev, void *stream) {
    return explain_call(model, lib, weights, nullptr, 1, ligands_dev, n, conf_max_dev, match_dev, levels_dev, best_conformer_dev, status_dev, stream);
}

extern "C" int pmx_explain_constrained(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const pmx_match_constraint *constraint,
                                       const uint64_t *ligands_dev, uint32_t n, double *conf_max_dev, uint8_t *match_dev, uint8_t *levels_dev,
                                       int32_t *best_conformer_dev, int32_t *status_dev, void *stream) {
    return explain_call(model, lib, weights, constraint, 1, ligands_dev, n, conf_max_dev, match_dev, levels_dev, best_conformer_dev, status_dev, stream);
}

extern "C" int pmx_explain_modes(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const pmx_match_constraint *constraint,
                                 int n_modes, const uint64_t *ligands_dev, uint32_t n, double *mode_max_dev, uint8_t *mode_match_dev, uint8_t *levels_dev,
                                 int32_t *best_conformer_dev, int32_t *status_dev, void *stream) {
    if (n_modes < 1 || n_modes > PMX_MAX_MODES) return pmx_fail(PMX_ERR_INVALID, "%d modes (1 to %d)", n_modes, PMX_MAX_MODES);
    return explain_call(model, lib, weights, constraint, n_modes, ligands_dev, n, mode_max_dev, mode_match_dev, levels_dev, best_conformer_dev, status_dev, stream);
}

// ------------------------------------------------------------------------------------ the row kernels (pmx_rows.hip)
// pmx_attribute, pmx_align and pmx_hotspots: one kernel over the call's rows; no tables, no slices, no arena. Of the workspace of (device, stream) it
// takes the CU count and four bytes for its row cursor, cleared in stream order in front of the launch. `what`: the call's name in a
// message; null_out: one of the caller's own device pointers is null; launch(blocks, p, cursor) starts the caller's kernel.
template <class Launch>
static int row_call(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], uint32_t n, const char *what, bool null_out,
                    pmx_rows::Kind kind, hipStream_t stream, Launch launch) {
    if (!model || !lib || !weights) return pmx_fail(PMX_ERR_INVALID, "null argument");
    if (n > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "more than %d rows in one %s call", PMX_EXPLAIN_MAX, what);
    if (n == 0) return PMX_OK;
    if (null_out) return pmx_fail(PMX_ERR_INVALID, "null argument");
    if (model->device != lib->device) return pmx_fail(PMX_ERR_INVALID, "model and library live on different devices");
    PMX_HIPCHECK(hipSetDevice(lib->device));
    const HeldWs held = hold_screen(lib->device, stream);
    ScreenWs &ws = *held.ws;
    const int rc = init_workspace(ws, lib->device, stream);
    if (rc) return rc;
    PMX_HIPCHECK(ws.acur.grow(256, stream));
    PMX_HIPCHECK(hipMemsetAsync(ws.acur.ptr, 0, 4, stream));
    const ScreenParams p = row_params(model, lib, weights);
    const unsigned per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(kLdsPerCu / pmx_rows::lds_bytes(kind), 8));
    const unsigned blocks = std::min<unsigned>(n, (unsigned)ws.num_cu * per_cu);
    launch(blocks, p, ws.acur.as<uint32_t>());
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_attribute(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const uint64_t *ligands_dev,
                             const int32_t *conformer_dev, const uint8_t *key_dev, uint32_t n, double *total_dev, double *node_dev, float *entry_dev,
                             uint16_t *fails_dev, uint8_t *levels_dev, int32_t *status_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool null_out = !ligands_dev || !conformer_dev || !key_dev || !total_dev || !node_dev || !entry_dev || !fails_dev || !levels_dev || !status_dev;
    return row_call(model, lib, weights, n, "attribute", null_out, pmx_rows::kAttribute, stream, [&](unsigned blocks, const ScreenParams &p, uint32_t *cursor) {
        const pmx_rows::AttributeArgs a{{ligands_dev, conformer_dev, key_dev, n, levels_dev, status_dev, cursor}, total_dev, node_dev, entry_dev, fails_dev};
        pmx_rows::launch(blocks, stream, p, a);
    });
}

extern "C" int pmx_hotspots(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const uint64_t *ligands_dev,
                            const int32_t *conformer_dev, const uint8_t *key_dev, uint32_t n, double *total_dev, double *hotspot_dev, uint32_t *terms_dev,
                            uint32_t *pass_dev, uint64_t *fingerprint_dev, uint8_t *levels_dev, int32_t *status_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool null_out = !ligands_dev || !conformer_dev || !key_dev || !total_dev || !hotspot_dev || !terms_dev || !pass_dev || !fingerprint_dev || !levels_dev || !status_dev;
    return row_call(model, lib, weights, n, "hotspots", null_out, pmx_rows::kHotspots, stream, [&](unsigned blocks, const ScreenParams &p, uint32_t *cursor) {
        const pmx_rows::HotspotArgs a{{ligands_dev, conformer_dev, key_dev, n, levels_dev, status_dev, cursor}, total_dev, hotspot_dev, terms_dev, pass_dev, fingerprint_dev};
        pmx_rows::launch(blocks, stream, p, a);
    });
}

extern "C" int pmx_align(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const double *node_center_dev,
                         const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint8_t *key_dev, uint32_t n, double *rot_dev, double *trans_dev,
                         double *fit_dev, double *node_dev, int32_t *count_dev, uint8_t *levels_dev, int32_t *status_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool null_out = !node_center_dev || !ligands_dev || !conformer_dev || !key_dev || !rot_dev || !trans_dev || !fit_dev || !node_dev || !count_dev || !levels_dev || !status_dev;
    return row_call(model, lib, weights, n, "align", null_out, pmx_rows::kAlign, stream, [&](unsigned blocks, const ScreenParams &p, uint32_t *cursor) {
        const pmx_rows::AlignArgs a{{ligands_dev, conformer_dev, key_dev, n, levels_dev, status_dev, cursor}, node_center_dev, rot_dev, trans_dev, fit_dev, node_dev, count_dev};
        pmx_rows::launch(blocks, stream, p, a);
    });
}
