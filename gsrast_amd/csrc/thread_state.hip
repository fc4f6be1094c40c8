// What a host thread's calls keep between them: the per-thread, per-device resources of gsr_forward (Readback: pinned words,
// events, the second stream), the tile histories with their entry points, the device's shape and the environment knobs.
#include <stdlib.h>

#include <map>

#include "api_internal.hpp"

namespace gsr {
namespace {
constexpr uint32_t kHistoryMagic = 0x54485347u;   // "GSHT"
constexpr size_t kMaxDefaultHistories = 8;        // streams per host thread and device that get a history of the library's own

int tile_history_new(gsr_tile_history** out) {
    gsr_tile_history* h = new gsr_tile_history;
    auto fail_with = [&](hipError_t e, const char* what) {
        set_hip_error(e, what);
        if (h->ticks[0]) (void)hipFree(h->ticks[0]);
        if (h->stats) (void)hipHostFree(h->stats);
        if (h->ev_order) (void)hipEventDestroy(h->ev_order);
        if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
        delete h;
        return GSR_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipGetDevice(&h->device)) != hipSuccess) return fail_with(e, "hipGetDevice");
    uint32_t* dev = nullptr;
    if ((e = hipMalloc(reinterpret_cast<void**>(&dev), sizeof(uint32_t) * (3 * kTileOrderMax + 32))) != hipSuccess) return fail_with(e, "hipMalloc (tile history)");
    h->ticks[0] = dev; h->ticks[1] = dev + kTileOrderMax; h->order = dev + 2 * kTileOrderMax; h->deep = dev + 3 * kTileOrderMax;
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&h->stats), 64, hipHostMallocMapped)) != hipSuccess) return fail_with(e, "hipHostMalloc (tile history)");
    memset(h->stats, 0, 64);
    if ((e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->stats_dev), h->stats, 0)) != hipSuccess) return fail_with(e, "hipHostGetDevicePointer");
    if ((e = hipEventCreateWithFlags(&h->ev_order, hipEventDisableTiming)) != hipSuccess) return fail_with(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming)) != hipSuccess) return fail_with(e, "hipEventCreate");
    h->magic = kHistoryMagic;
    *out = h;
    return GSR_OK;
}

void destroy_history(gsr_tile_history* h) {
    h->magic = 0;
    (void)hipFree(h->ticks[0]);
    (void)hipHostFree(h->stats);
    (void)hipEventDestroy(h->ev_order);
    (void)hipEventDestroy(h->ev_switch);
    delete h;
}
}  // namespace

int Readback::ensure() {
    if (!host) {
        const size_t bytes = sizeof(uint32_t) * kHostWords;
        GSR_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&host), bytes, hipHostMallocMapped));
        memset(host, 0, bytes);
        GSR_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&host_dev), host, 0));
        staged_host = reinterpret_cast<unsigned long long*>(host + kHostStaged);
    }
    if (!ev_r) GSR_HIP_TRY(hipEventCreateWithFlags(&ev_r, hipEventDisableTiming));
    return GSR_OK;
}
int Readback::ensure_side() {
    if (!side) {
        // (a priority of its own: HIP maps the streams of a priority onto a few hardware queues, and in a process with
        // many streams — torch.distributed and RCCL bring theirs — this one landed on the caller's queue: its kernels then
        // ran in front of the caller's instead of beside them, forced-distributed bench 1.37 -> 1.45 ms. The lower
        // priority also suits what it carries: work that is to fill gaps, never to be waited for)
        // (measured, forced-distributed / plain bench: normal 1.441 / 1.211, lowest 1.214 / 1.208, highest 1.237 / 1.243 ms)
        int prio_low = 0, prio_high = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_low, &prio_high) != hipSuccess) { (void)hipGetLastError(); prio_low = 0; }
        GSR_HIP_TRY(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, prio_low));
        GSR_HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        GSR_HIP_TRY(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    }
    return GSR_OK;
}
int Readback::ensure_colors() {
    { const int rc = ensure_side(); if (rc != GSR_OK) return rc; }
    if (!ev_colors) {
        GSR_HIP_TRY(hipEventCreateWithFlags(&ev_colors, hipEventDisableTiming));
        GSR_HIP_TRY(hipEventCreateWithFlags(&ev_pre_blend, hipEventDisableTiming));
    }
    return GSR_OK;
}
int Readback::ensure_staged() {
    if (!staged_dev) GSR_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&staged_dev), sizeof(unsigned long long)));
    return GSR_OK;
}
int Readback::ensure_events() {
    if (!events) {
        for (auto& e : ev) GSR_HIP_TRY(hipEventCreate(&e));
        events = true;
    }
    return GSR_OK;
}

namespace {
// Everything the calling thread owns, per device; given back by gsr_thread_release and when the thread ends.
struct ThreadResources {
    std::map<int, Readback> by_device;
    void release();
    ~ThreadResources() { release(); }
};
static thread_local ThreadResources g_thread;

// The environment switches (EnvKnobs, frame_policy.hpp): read once per process, before the first call needs them.
EnvKnobs read_env_knobs() {
    EnvKnobs e;
    const char* h = getenv("GSR_TILE_HISTORY");
    e.tile_history = !(h && h[0] == '0');
    const char* c = getenv("GSR_COLORS_BESIDE");
    e.colors_beside = c && c[0] >= '0' && c[0] <= '2' ? c[0] - '0' : -1;
    const char* f = getenv("GSR_FUSED_DEPTH");
    e.fused_depth = f && (f[0] == '0' || f[0] == '1') ? f[0] - '0' : -1;
    const char* ce = getenv("GSR_COLORS_EARLY_PCT");
    e.colors_early_pct = ce && ce[0] >= '0' && ce[0] <= '9' ? std::min(100, atoi(ce)) : -1;
    const char* dr = getenv("GSR_DEPTH_RECORDS");
    e.depth_records = dr && (dr[0] == '0' || dr[0] == '1') ? dr[0] - '0' : -1;
    const char* dh = getenv("GSR_DEEP_BY_HISTORY");
    e.deep_by_history = dh && dh[0] == '1';
    const char* st = getenv("GSR_SORT_SINGLE_TICKET");
    e.sort_single_ticket = st && (st[0] == '0' || st[0] == '1') ? st[0] - '0' : -1;
    return e;
}
// (read when the first call needs them; gsr_reread_environment — the tests' and A/B scripts' way of changing a knob inside one
// process — reads them again: no call may be in flight on another thread meanwhile)
EnvKnobs& env_knobs_storage() {
    static EnvKnobs k = read_env_knobs();
    return k;
}
}  // namespace

const EnvKnobs& env_knobs() { return env_knobs_storage(); }

// The calling thread's resources for the CURRENT device.
int current_readback(Readback*& out) {
    int dev = 0;
    GSR_HIP_TRY(hipGetDevice(&dev));
    out = &g_thread.by_device[dev];
    return GSR_OK;
}

// The call's tile history: the caller's own, or this thread's for the call's stream (none: *out = nullptr).
int history_of_call(const gsr_forward_args& a, const FrameDims& d, bool enabled, hipStream_t stream, Readback& rb,
                    gsr_tile_history** out) {
    gsr_tile_history*& hist = *out;
    hist = nullptr;
    if (!enabled || (a.flags & GSR_FLAG_NO_TILE_HISTORY) || tile_order_workgroups(d) > kTileOrderMax ||
        d.grid_x * d.grid_y > kTileOrderMax)
        return GSR_OK;
    if (a.tile_history) {
        int dev_now = -1;
        GSR_HIP_TRY(hipGetDevice(&dev_now));
        if (a.tile_history->magic != kHistoryMagic || a.tile_history->device != dev_now) return GSR_ERR_INVALID_ARG;
        hist = a.tile_history;
        if (hist->used && hist->last_stream != stream) {
            // (the caller has taken its history to another stream: this call's kernels go behind what the old stream holds
            // now — if that stream is gone, so is its work)
            if (hipEventRecord(hist->ev_switch, hist->last_stream) == hipSuccess) GSR_HIP_TRY(hipStreamWaitEvent(stream, hist->ev_switch, 0));
            else (void)hipGetLastError();
        }
    } else {
        for (gsr_tile_history* h : rb.default_histories)
            if (h->last_stream == stream) { hist = h; break; }
        if (!hist && rb.default_histories.size() >= kMaxDefaultHistories) {
            // A ninth stream: the history this thread has not used for the longest time goes — its stream may be gone
            // (a caller that makes a stream per frame), so nothing is asked of that stream: freeing the history's memory
            // waits for the device to be done with it (hipFree). Rare by construction; before round 6 the calls on
            // further streams simply ran without a history, for good.
            size_t lru = 0;
            for (size_t i = 1; i < rb.default_histories.size(); ++i)
                if ((int32_t)(rb.default_histories[i]->last_serial - rb.default_histories[lru]->last_serial) < 0) lru = i;
            destroy_history(rb.default_histories[lru]);
            rb.default_histories.erase(rb.default_histories.begin() + (long)lru);
        }
        if (!hist) {
            // (a history is an accelerator: if the device has no memory left for one, the call runs without)
            if (tile_history_new(&hist) == GSR_OK) rb.default_histories.push_back(hist);
            else { hist = nullptr; (void)hipGetLastError(); clear_hip_error(); }
        }
    }
    if (hist) { hist->last_stream = stream; hist->used = true; hist->last_serial = rb.serial; return rb.ensure_side(); }       // (the stream the sort of the order runs on)
    return GSR_OK;
}

// Gives back what the calling thread's calls have made the library allocate, for every device: the second stream (drained
// first: nothing of the library's is in flight afterwards — work on the CALLER's streams is the caller's to wait for before
// it frees the chunks), the pinned words, every event, the staged-record counter and the histories the library kept for
// calls without one of their own. A later call of the thread starts from nothing again.
void ThreadResources::release() {
    if (by_device.empty()) return;
    int before = -1;
    const bool have_device = hipGetDevice(&before) == hipSuccess;
    for (auto& kv : by_device) {
        Readback& rb = kv.second;
        if (hipSetDevice(kv.first) != hipSuccess) { (void)hipGetLastError(); continue; }     // (the runtime is gone: nothing left to free)
        if (rb.side) { (void)hipStreamSynchronize(rb.side); (void)hipStreamDestroy(rb.side); }
        for (gsr_tile_history* h : rb.default_histories) destroy_history(h);
        if (rb.events) for (auto& e : rb.ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : {rb.ev_r, rb.ev_fork, rb.ev_join, rb.ev_colors, rb.ev_pre_blend})
            if (e) (void)hipEventDestroy(e);
        if (rb.staged_dev) (void)hipFree(rb.staged_dev);
        if (rb.host) (void)hipHostFree(rb.host);
        (void)hipGetLastError();
    }
    by_device.clear();
    if (have_device) (void)hipSetDevice(before);
    (void)hipGetLastError();
}

const uint32_t* tile_order_of_call(const gsr_forward_receipt& r, int row_begin, int row_end) {
    if (r.serial == 0u) return nullptr;
    const int dims[4] = {r.width, r.height, row_begin, row_end};
    auto fits = [&](const gsr_tile_history* h) {
        return h && h->magic == kHistoryMagic && h->order_serial == r.serial && memcmp(dims, h->dims, sizeof(dims)) == 0;
    };
    if (r.tile_history) return fits(r.tile_history) ? r.tile_history->order : nullptr;    // (the caller's own: its to share between threads)
    Readback* rb = nullptr;
    if (current_readback(rb) != GSR_OK) return nullptr;
    for (const gsr_tile_history* h : rb->default_histories)
        if (fits(h)) return h->order;
    return nullptr;
}

int current_device_shape(DeviceShape* out) {
    static thread_local std::map<int, DeviceShape> cache;
    int dev = 0;
    GSR_HIP_TRY(hipGetDevice(&dev));
    auto it = cache.find(dev);
    if (it == cache.end()) {
        int cus = 0;
        GSR_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        it = cache.emplace(dev, device_shape_of(cus)).first;
    }
    *out = it->second;
    return GSR_OK;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

static int tile_history_create_impl(gsr_tile_history** out) {
    if (!out) return GSR_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GSR_ERR_NO_DEVICE;
    return tile_history_new(out);
}
int gsr_tile_history_create(gsr_tile_history** out) { return entry_point(tile_history_create_impl, out); }

static int tile_history_destroy_impl(gsr_tile_history* h) {
    if (!h) return GSR_OK;
    if (h->magic != kHistoryMagic) return GSR_ERR_INVALID_ARG;
    destroy_history(h);
    return GSR_OK;
}
int gsr_tile_history_destroy(gsr_tile_history* h) { return entry_point(tile_history_destroy_impl, h); }

void gsr_reread_environment(void) { env_knobs_storage() = read_env_knobs(); }

static int thread_release_impl() { g_thread.release(); return GSR_OK; }
int gsr_thread_release(void) { return entry_point(thread_release_impl); }

void gsr_device_shape(int cus, uint32_t out[4]) {
    const DeviceShape s = device_shape_of(cus);
    out[0] = (uint32_t)s.cus; out[1] = s.blend_slots; out[2] = s.blend_slots_beside; out[3] = (uint32_t)(s.light_frame_ticks / 25000ull);
}

static int tile_history_stats_impl(const gsr_tile_history* h, uint32_t* out) {
    if (!h || h->magic != kHistoryMagic || !out) return GSR_ERR_INVALID_ARG;
    out[0] = h->stats[0] != 0u ? h->stats[2] : h->view.mean;          // (words the last sort has left and no call has read yet come first)
    out[1] = h->stats[1];
    out[2] = h->stats[3];
    out[3] = (h->stats[0] != 0u ? h->stats[4] != 0u : h->view.decorrelated) ? 1u : 0u;
    out[4] = h->view.calls;
    out[5] = h->view.overlapped ? 1u : 0u;
    return GSR_OK;
}
int gsr_tile_history_stats(const gsr_tile_history* h, uint32_t out[6]) { return entry_point(tile_history_stats_impl, h, out); }

static int tile_history_forget_stream_impl(gsr_tile_history* h) {
    if (!h || h->magic != kHistoryMagic) return GSR_ERR_INVALID_ARG;
    h->used = false;
    h->last_stream = nullptr;
    return GSR_OK;
}
int gsr_tile_history_forget_stream(gsr_tile_history* h) { return entry_point(tile_history_forget_stream_impl, h); }

static int tile_history_times_impl(const gsr_tile_history* h, uint32_t* times, int count, uint32_t* deep_tiles) {
    if (!h || h->magic != kHistoryMagic || !times || count < 0 || count > kTileOrderMax) return GSR_ERR_INVALID_ARG;
    // (a tool's call: it synchronises the device — the history's calls may be on any stream)
    GSR_HIP_TRY(hipDeviceSynchronize());
    GSR_HIP_TRY(hipMemcpy(times, h->ticks[h->cur ^ 1], sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToHost));
    if (deep_tiles) GSR_HIP_TRY(hipMemcpy(deep_tiles, h->deep, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return GSR_OK;
}
int gsr_tile_history_times(const gsr_tile_history* h, uint32_t* times, int count, uint32_t* deep_tiles) {
    return entry_point(tile_history_times_impl, h, times, count, deep_tiles);
}

}  // extern "C"
