// C-ABI of libmfa_hip.so (include/mfa_hip.h): glue between plain-C callers and the kernels.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "mfa_internal.h"
#include "dfa_spec_core.h"

namespace mfa {

static thread_local int g_last_hip_error = 0;
void set_last_hip_error(int e) { g_last_hip_error = e; }

int check_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return MFA_ERR_NO_DEVICE;
    HIP_TRY(hipSetDevice(device));
    return MFA_OK;
}

static void ctx_free(LaunchCtx& cx) {
    if (cx.d_counter) (void)hipFree(cx.d_counter);
    lean_hint_free(cx.lean);
    if (cx.d_scratch) (void)hipFree(cx.d_scratch);
    if (cx.d_regions) (void)hipFree(cx.d_regions);
    if (cx.d_split) (void)hipFree(cx.d_split);
    if (cx.split_seen) (void)hipHostFree(cx.split_seen);
    for (void* ev : {cx.ev_start, cx.ev_stop, cx.ev_r0, cx.ev_r1, cx.ev_done})
        if (ev) (void)hipEventDestroy((hipEvent_t)ev);
    cx = LaunchCtx{};
}

// grow *buf to `need` bytes (contents are not kept).  Frees the old buffer first: hipFree waits for the device, so a
// kernel of an earlier launch on the same stream that still uses it has finished by then.
int ctx_reserve(void** buf, size_t* have, size_t need) {
    if (need <= *have) return MFA_OK;
    if (*buf) HIP_TRY(hipFree(*buf));
    *buf = nullptr; *have = 0;
    const size_t want = need + need / 4;                      // head room: batches of similar size do not reallocate
    hipError_t e = hipMalloc(buf, want);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {      // not with head room: exactly what is needed, or an honest "no memory"
        (void)hipGetLastError();
        e = hipMalloc(buf, need);
        if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) { (void)hipGetLastError(); *buf = nullptr; set_last_hip_error((int)e); return MFA_ERR_NOMEM; }
        if (e == hipSuccess) { *have = need; return MFA_OK; }
    }
    if (e != hipSuccess) { *buf = nullptr; set_last_hip_error((int)e); return MFA_ERR_HIP; }
    *have = want;
    return MFA_OK;
}

// A context for a launch on `stream`: the one this stream used last (its work is ordered before ours), else one whose
// last launch has completed, else a new one.  The caller holds the image mutex and has set the device.
int ctx_acquire(DeviceState& ds, void* stream, LaunchCtx** out) {
    LaunchCtx* pick = nullptr;
    for (LaunchCtx* cx : ds.ctxs)
        if (cx->used && cx->stream == stream) { pick = cx; break; }
    if (!pick)
        for (LaunchCtx* cx : ds.ctxs)
            if (!cx->used || hipEventQuery((hipEvent_t)cx->ev_done) == hipSuccess) { pick = cx; break; }
    if (!pick && ds.ctxs.size() >= 64) {                       // far more overlapping launches than a device runs at once: wait for the oldest
        pick = ds.ctxs.front();
        HIP_TRY(hipEventSynchronize((hipEvent_t)pick->ev_done));
    }
    if (!pick) {
        LaunchCtx* cx = new (std::nothrow) LaunchCtx();
        if (!cx) return MFA_ERR_NOMEM;
        hipError_t e = hipMalloc((void**)&cx->d_counter, 256 + (getenv("MFA_STATS") ? (4u << 20) : 0));
        if (e == hipSuccess) e = hipEventCreate((hipEvent_t*)&cx->ev_start);
        if (e == hipSuccess) e = hipEventCreate((hipEvent_t*)&cx->ev_stop);
        if (e == hipSuccess) e = hipEventCreate((hipEvent_t*)&cx->ev_r0);
        if (e == hipSuccess) e = hipEventCreate((hipEvent_t*)&cx->ev_r1);
        if (e == hipSuccess) e = hipEventCreateWithFlags((hipEvent_t*)&cx->ev_done, hipEventDisableTiming);
        if (e != hipSuccess) { set_last_hip_error((int)e); ctx_free(*cx); delete cx; return MFA_ERR_HIP; }
        ds.ctxs.push_back(cx);
        pick = cx;
    }
    pick->used = true; pick->stream = stream; pick->ran_regions = false; pick->split_ran = false; pick->spec_ran = false; pick->set_split_ran = false;
    ds.last = pick;
    *out = pick;
    return MFA_OK;
}

void device_release(DeviceState& ds) {
    if (ds.device < 0) return;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return;
    (void)hipSetDevice(ds.device);
    if (ds.d_dfa_trans) (void)hipFree(ds.d_dfa_trans);
    if (ds.d_dfa_accept) (void)hipFree(ds.d_dfa_accept);
    if (ds.d_byte_class) (void)hipFree(ds.d_byte_class);
    if (ds.d_set_tables) (void)hipFree(ds.d_set_tables);
    if (ds.d_set_home) (void)hipFree(ds.d_set_home);
    if (ds.d_walk) (void)hipFree(ds.d_walk);
    for (uint16_t* t : ds.d_search)
        if (t) (void)hipFree(t);
    for (LaunchCtx* cx : ds.ctxs) { ctx_free(*cx); delete cx; }
    jit_unload(ds);
    ds = DeviceState{};
    (void)hipSetDevice(cur);
}

// caller holds img->mu
int device_prepare(mfa_image* img, int device, DeviceState** out) {
    int rc = check_device(device);
    if (rc != MFA_OK) return rc;
    auto it = img->dev.find(device);
    if (it != img->dev.end()) { *out = &it->second; return MFA_OK; }
    DeviceState ds;
    ds.device = device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    ds.n_cus = prop.multiProcessorCount;
    const HostImage& h = img->host;
    auto up = [&](void** dst, const void* src, size_t bytes) -> int {
        HIP_TRY(hipMalloc(dst, bytes ? bytes : 4));
        if (bytes) HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return MFA_OK;
    };
    if (h.h.kind == MFA_KIND_MFA) {
        if (img->walk_ok) rc = up((void**)&ds.d_walk, img->walk.words.data(), img->walk.words.size() * 4);
    } else if (h.set_walk) {
        rc = up((void**)&ds.d_set_tables, h.set_tables.data(), h.set_tables.size() * 4);
        if (rc == MFA_OK && h.set_wave) rc = up((void**)&ds.d_set_home, h.set_home_wide, sizeof h.set_home_wide);      // (the table layout stays as it is)
    } else {
        if (h.dfa_states <= 0xffffu) {
            std::vector<uint16_t> t16(h.dfa_trans.begin(), h.dfa_trans.end());
            rc = up((void**)&ds.d_dfa_trans, t16.data(), t16.size() * 2);
        } else rc = up((void**)&ds.d_dfa_trans, h.dfa_trans.data(), h.dfa_trans.size() * 4);
        if (rc == MFA_OK) rc = up((void**)&ds.d_dfa_accept, h.dfa_accept.data(), h.dfa_accept.size());
        if (rc == MFA_OK) rc = up((void**)&ds.d_byte_class, h.byte_class, 256);
    }
    if (rc != MFA_OK) { device_release(ds); return rc; }
    auto ins = img->dev.emplace(device, ds);
    *out = &ins.first->second;
    return MFA_OK;
}

// A batch given with HOST pointers: checks it, copies it to the device (offsets relative to the first string), runs `match` on the copies,
// copies the results back and synchronises (throughput is then bounded by the host link).  states != NULL (the resume calls' host forms):
// n records of state_bytes each (one word, or a mfa_set_state) that travel to the device and back as well; `results` may then be NULL.
// check_lengths: refuse strings beyond the limit.
int match_host_staged(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results, int device, const HostMatch& match, void* states, size_t state_bytes,
                      bool check_lengths) {
    if (!offsets || (!results && !states && n)) return MFA_ERR_INVALID_ARG;
    if (n == 0) return MFA_OK;
    for (uint64_t k = 0; k < n; k++) {
        if (offsets[k + 1] < offsets[k]) return MFA_ERR_INVALID_ARG;
        if (check_lengths && offsets[k + 1] - offsets[k] > MFA_MAX_STRING_BYTES) return MFA_ERR_TOO_LONG;
    }
    int rc = check_device(device);
    if (rc != MFA_OK) return rc;
    const uint64_t total = offsets[n] - offsets[0];
    uint8_t* d_bytes = nullptr; uint64_t* d_off = nullptr; void* d_st = nullptr; uint8_t* d_res = nullptr;
    std::vector<uint64_t> rel(n + 1);
    for (uint64_t k = 0; k <= n; k++) rel[k] = offsets[k] - offsets[0];
    hipError_t e = hipMalloc((void**)&d_bytes, total + 64);
    if (e == hipSuccess) e = hipMalloc((void**)&d_off, (n + 1) * sizeof(uint64_t));
    if (e == hipSuccess && states) e = hipMalloc(&d_st, n * state_bytes);
    if (e == hipSuccess && results) e = hipMalloc((void**)&d_res, n);
    if (e == hipSuccess && total) e = hipMemcpy(d_bytes, bytes + offsets[0], total, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_off, rel.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && states) e = hipMemcpy(d_st, states, n * state_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_last_hip_error((int)e); rc = MFA_ERR_HIP; }
    if (rc == MFA_OK) rc = match(d_bytes, d_off, d_res, total, d_st);
    if (rc == MFA_OK) {
        e = hipDeviceSynchronize();
        if (e == hipSuccess && states) e = hipMemcpy(states, d_st, n * state_bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess && results) e = hipMemcpy(results, d_res, n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { set_last_hip_error((int)e); rc = MFA_ERR_HIP; }
    }
    for (void* p : {(void*)d_bytes, (void*)d_off, d_st, (void*)d_res})
        if (p) (void)hipFree(p);
    return rc;
}

// A launch: the image's lock, its state on the device and a context.  Whatever happens to a launch once it holds a context, the context's
// `done` event is recorded behind what was enqueued (before the lock goes): a launch on another stream must not be handed this context (its
// counter, scratch area and table) while a kernel of this call may still be using it
struct Launch {
    std::unique_lock<std::mutex> lk;
    DeviceState* ds = nullptr; LaunchCtx* cx = nullptr; void* stream = nullptr;
    ~Launch() { if (cx) (void)hipEventRecord((hipEvent_t)cx->ev_done, (hipStream_t)stream); }
};
// locks the image and prepares the device (unless L holds them already), takes the context for a launch on `stream`, notes which kernel walks
static int launch_open(mfa_image* img, int device, void* stream, uint32_t kernel, Launch& L) {
    int rc = MFA_OK;
    if (!L.ds) { L.lk = std::unique_lock<std::mutex>(img->mu); rc = device_prepare(img, device, &L.ds); }
    if (rc == MFA_OK) rc = ctx_acquire(*L.ds, stream, &L.cx);
    if (rc != MFA_OK) return rc;
    L.stream = stream; img->last_kernel = kernel;
    return MFA_OK;
}

// the workspace of the image's last launch on `device`, or nullptr; the caller holds img->mu
static LaunchCtx* last_ctx(mfa_image* img, int device) {
    auto it = img->dev.find(device);
    return it == img->dev.end() ? nullptr : it->second.last;
}

// the header words the split kernels of the image's last launch on `device` left (zeros when they did not run: `ran`)
static int last_split_header(mfa_image* img, int device, bool LaunchCtx::*ran, uint32_t (&h)[SPLIT_H_WORDS]) {
    if (!img) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(img->mu);
    LaunchCtx* cx = last_ctx(img, device);
    if (!cx) return MFA_ERR_INVALID_ARG;
    if (cx->*ran) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipEventSynchronize((hipEvent_t)cx->ev_done));
        HIP_TRY(hipMemcpy(h, cx->d_split, sizeof h, hipMemcpyDeviceToHost));
    }
    return MFA_OK;
}

// what the plan kernel, and what the repair and resolve kernels, left in a header
static void split_words(const uint32_t (&h)[SPLIT_H_WORDS], uint64_t* strings, uint64_t* chunks, uint32_t* chunk_bytes) {
    if (strings) *strings = h[SPLIT_H_STRINGS];
    if (chunks) *chunks = h[SPLIT_H_CHUNKS];
    if (chunk_bytes) *chunk_bytes = h[SPLIT_H_STRINGS] ? h[SPLIT_H_CHUNK] : 0u;
}
static void spec_words(const uint32_t (&h)[SPLIT_H_WORDS], uint64_t* rewalked_chunks, uint64_t* serial_strings, uint64_t* serial_bytes) {
    if (rewalked_chunks) *rewalked_chunks = h[SPEC_H_REWALKED];
    if (serial_strings) *serial_strings = h[SPEC_H_SERIAL_STRINGS];
    if (serial_bytes) *serial_bytes = (uint64_t)h[SPEC_H_SERIAL_BYTES] | (uint64_t)h[SPEC_H_SERIAL_BYTES + 1u] << 32;
}

}  // namespace mfa

using namespace mfa;

extern "C" {

int mfa_image_create(const void* blob, size_t n_bytes, mfa_image_t** out) {
    if (!blob || !out) return MFA_ERR_INVALID_ARG;
    *out = nullptr;
    mfa_image* img = new (std::nothrow) mfa_image();
    if (!img) return MFA_ERR_NOMEM;
    int rc = parse_blob(blob, n_bytes, img->host);
    if (rc == MFA_OK) rc = img->host.h.kind == MFA_KIND_MFA ? check_mfa_invariants(img->host) : nfa_image_build(img->host);
    if (rc != MFA_OK) { delete img; return rc; }
    if (spec_applies(img->host)) img->host.dfa_home = spec_home_state(img->host.dfa_trans.data(), img->host.dfa_states, img->host.n_classes);
    if (img->host.h.kind == MFA_KIND_MFA) {
        img->walk_ok = build_walk_tables(img->host, img->walk) == MFA_OK;
        if (!img->walk_ok && !jit_enabled(img->host)) { delete img; return MFA_ERR_UNSUPPORTED; }      // no kernel could walk it
    }
    *out = img;
    return MFA_OK;
}

void mfa_image_destroy(mfa_image_t* img) {
    if (!img) return;
    for (auto& kv : img->dev) device_release(kv.second);
    delete img;
}

int mfa_image_get_info(const mfa_image_t* img, mfa_image_info* out) {
    if (!img || !out) return MFA_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    out->kind = img->host.h.kind; out->is_reversed = img->host.h.is_reversed;
    out->n_nodes = img->host.h.n_nodes; out->n_edges = img->host.h.n_edges; out->n_cells = img->host.h.n_cells;
    out->dfa_states = img->host.dfa_states; out->byte_classes = img->host.n_classes;
    out->last_kernel = img->last_kernel;
    return MFA_OK;
}

int mfa_image_prepare(mfa_image_t* img, int device) {
    if (!img) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(img->mu);
    DeviceState* ds = nullptr;
    int rc = device_prepare(img, device, &ds);
    if (rc == MFA_OK && img->host.h.kind == MFA_KIND_MFA && walk_mode() != 1 && (walk_mode() == 2 || !img->walk_ok || (jit_lanes(img->host) == 64u && jit_cached(img->host))))
        (void)jit_load(img->host, *ds);
    return rc;
}

int mfa_image_specialize(mfa_image_t* img) {
    if (!img) return MFA_ERR_INVALID_ARG;
    if (!jit_enabled(img->host)) return MFA_ERR_UNSUPPORTED;
    std::string err;
    if (jit_compile(img->host, &err).empty()) {
        fprintf(stderr, "mfa_hip: %s\n", err.c_str());
        return MFA_ERR_JIT;
    }
    return MFA_OK;
}

// own_regions: run the region pass into the context's table; else use d_table (may be NULL)
static int match_impl(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint8_t* d_results,
                      const uint64_t* d_table, bool own_regions, int device, void* stream) {
    if (!img || !d_offsets || (!d_results && n)) return MFA_ERR_INVALID_ARG;
    if (n == 0) return MFA_OK;
    Launch L;
    L.lk = std::unique_lock<std::mutex>(img->mu);
    int rc = device_prepare(img, device, &L.ds);
    if (rc != MFA_OK) return rc;
    DeviceState* ds = L.ds;
    const bool is_mfa = img->host.h.kind == MFA_KIND_MFA;
    // Which walk: the table-driven kernel (walk.hip) works for every automaton at once; a kernel generated for this automaton
    // (jit_gen.cpp) steps faster on small automata but has to be compiled first.  Automatic: the generated kernel if its code object
    // is in the cache already (mfa_image_specialize builds it ahead of time), is not of the "huge" kind, and MFA_JIT != 0 -- a
    // match call never waits for a compiler.  MFA_WALK=table / MFA_WALK=jit force one or the other (jit compiles on demand).
    const int mode = walk_mode();
    bool want_jit = false;
    if (is_mfa) {
        if (mode == 2 || !img->walk_ok) want_jit = jit_enabled(img->host);
        else if (mode == 0) {
            if (!ds->jit_tried && !ds->jit_probed) { ds->jit_probed = true; ds->jit_in_cache = jit_lanes(img->host) == 64u && jit_cached(img->host); }
            want_jit = ds->jit_fn != nullptr || ds->jit_in_cache;
        }
    }
    const bool jit = want_jit && jit_load(img->host, *ds);
    const bool table_walk = is_mfa && !jit && img->walk_ok;
    if (is_mfa && !jit && !table_walk) return MFA_ERR_JIT;      // only a generated kernel could walk it, and none could be built
    // MFA_REQUIRE_JIT=1: a caller that counts on the specialised kernel's step rate gets an error instead of the other engine;
    // MFA_VERBOSE=1: which kernel walks, on stderr
    if (is_mfa && !jit) { const char* rq = getenv("MFA_REQUIRE_JIT"); if (rq && rq[0] == '1') return MFA_ERR_JIT; }
    if (const char* vb = getenv("MFA_VERBOSE"))
        if (vb[0] == '1') fprintf(stderr, "mfa_hip: %s\n", !is_mfa ? img->host.set_wave ? "set walk of the automaton's nodes, one string per wave (nfa_set_wave_kernel)" : img->host.set_walk ? "set walk of the automaton's nodes (nfa_set_kernel)" : "table walk of the tabulated automaton (dfa_*_kernel)" : jit ? "kernel generated for this automaton (mfa_jit_kernel)" : "table-driven walk (walk_kernel)");
    rc = launch_open(img, device, stream, table_walk ? MFA_KERNEL_WALK : jit ? MFA_KERNEL_SPECIALISED : img->host.set_walk ? MFA_KERNEL_NODESET : MFA_KERNEL_TABLE, L);
    if (rc != MFA_OK) return rc;
    LaunchCtx* cx = L.cx;
    if (is_mfa && own_regions && regions_enabled()) {
        rc = ctx_reserve((void**)&cx->d_regions, &cx->region_bytes, (size_t)n * MFA_REGION_WORDS * sizeof(uint64_t));
        if (rc != MFA_OK) return rc;
        HIP_TRY(hipEventRecord((hipEvent_t)cx->ev_r0, (hipStream_t)stream));
        rc = launch_region_scan(ds->n_cus, d_bytes, d_offsets, n, cx->d_regions, stream);
        if (rc != MFA_OK) return rc;
        HIP_TRY(hipEventRecord((hipEvent_t)cx->ev_r1, (hipStream_t)stream));
        cx->ran_regions = true;
        d_table = cx->d_regions;
    }
    if (table_walk) {
        const WalkPlanInput p{img->walk.K, img->walk.max_live, img->walk.reversed, (uint32_t)img->walk.words.size()};
        const uint32_t sf[2] = {0u, (uint32_t)n}, stb[1] = {0u};
        if (n > 0xffffffffull) return MFA_ERR_INVALID_ARG;
        HIP_TRY(hipEventRecord((hipEvent_t)cx->ev_start, (hipStream_t)stream));
        rc = launch_walk(p, ds->d_walk, ds->n_cus, d_bytes, d_offsets, n, d_results, d_table, 1u, sf, stb, &cx->d_scratch, &cx->scratch_bytes,
                         cx->d_counter, stream, &cx->lean);
        HIP_TRY(hipEventRecord((hipEvent_t)cx->ev_stop, (hipStream_t)stream));
    } else if (jit) {
        rc = launch_mfa_jit(*ds, *cx, d_bytes, d_offsets, n, d_results, d_table, stream);
    } else {
        rc = launch_dfa_walk(img->host, *ds, *cx, d_bytes, d_offsets, n, d_results, stream);
    }
    return rc;
}

int mfa_match_batch(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint8_t* d_results,
                    int device, void* stream) {
    return match_impl(img, d_bytes, d_offsets, n, d_results, nullptr, true, device, stream);
}

int mfa_match_batch_regions(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint8_t* d_results,
                            const uint64_t* d_table, int device, void* stream) {
    return match_impl(img, d_bytes, d_offsets, n, d_results, d_table, false, device, stream);
}

int mfa_region_scan(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint64_t* d_table, int device, void* stream) {
    if (!d_offsets || (!d_table && n)) return MFA_ERR_INVALID_ARG;
    if (n == 0) return MFA_OK;
    const int rc = check_device(device);
    if (rc != MFA_OK) return rc;
    static int cus[64] = {0};
    if (device < 64 && cus[device] == 0) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        cus[device] = prop.multiProcessorCount;
    }
    return launch_region_scan(device < 64 ? cus[device] : 256, d_bytes, d_offsets, n, d_table, stream);
}

int mfa_match_batch_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results,
                         int device) {
    if (!img) return MFA_ERR_INVALID_ARG;
    return match_host_staged(bytes, offsets, n, results, device, [&](const uint8_t* d_bytes, const uint64_t* d_off, uint8_t* d_res, uint64_t, void*) {
        return mfa_match_batch(img, d_bytes, d_off, n, d_res, device, nullptr); });
}

int mfa_match_batch_resume(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint32_t* d_states,
                           uint8_t* d_results, int device, void* stream) {
    if (!img || !d_offsets) return MFA_ERR_INVALID_ARG;
    if (img->host.h.kind != MFA_KIND_NFA) return MFA_ERR_UNSUPPORTED;      // a memory automaton's state holds spans of the input: nothing to hand over
    if (img->host.set_walk) return MFA_ERR_UNSUPPORTED;                    // a set-walk image's state is a set of nodes, not one 32-bit number
    if (!d_states) return MFA_ERR_INVALID_ARG;
    if (n == 0) return MFA_OK;
    Launch L;
    const int rc = launch_open(img, device, stream, MFA_KERNEL_TABLE, L);
    if (rc != MFA_OK) return rc;
    return launch_dfa_resume(img->host, *L.ds, *L.cx, d_bytes, d_offsets, n, d_states, d_results, stream);
}

// host pointers: stage the pieces and the states, match, copy states (and results, unless NULL) back, synchronise.  No length check
// here: a piece beyond the limit is the device's sticky error, not a refused call.
int mfa_match_batch_resume_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t* states, uint8_t* results,
                                int device) {
    if (!img || !offsets) return MFA_ERR_INVALID_ARG;
    if (img->host.h.kind != MFA_KIND_NFA || img->host.set_walk) return MFA_ERR_UNSUPPORTED;
    if (!states) return MFA_ERR_INVALID_ARG;
    return match_host_staged(bytes, offsets, n, results, device, [&](const uint8_t* d_bytes, const uint64_t* d_off, uint8_t* d_res, uint64_t, void* d_st) {
        return mfa_match_batch_resume(img, d_bytes, d_off, n, (uint32_t*)d_st, d_res, device, nullptr); }, states, sizeof(uint32_t), false);
}

static_assert(sizeof(mfa_set_state) == 48 && offsetof(mfa_set_state, nodes) == 16, "a record is three 16-byte quarters: tag and reserved, nodes[0..3], nodes[4..7]");

int mfa_match_batch_resume_set(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, mfa_set_state* d_states,
                               uint8_t* d_results, int device, void* stream) {
    if (!img || !d_offsets || !d_states) return MFA_ERR_INVALID_ARG;
    if (img->host.h.kind != MFA_KIND_NFA) return MFA_ERR_UNSUPPORTED;      // a memory automaton's state holds spans of the input: nothing to hand over
    if (!img->host.set_walk) return MFA_ERR_UNSUPPORTED;                   // a tabulated image's state is one number: mfa_match_batch_resume
    if (img->host.set_wave) return MFA_ERR_UNSUPPORTED;                    // a wave image's set may take 64 words, a record has eight: the records are left as they came
    if ((uintptr_t)d_states & 15u) return MFA_ERR_INVALID_ARG;             // the kernel reads and writes a record as 16-byte quarters
    if (n == 0) return MFA_OK;
    Launch L;
    const int rc = launch_open(img, device, stream, MFA_KERNEL_NODESET, L);
    if (rc != MFA_OK) return rc;
    return launch_nfa_set_resume(img->host, *L.ds, *L.cx, d_bytes, d_offsets, n, reinterpret_cast<uint32_t*>(d_states), d_results, stream);
}

// host pointers: as mfa_match_batch_resume_host, with records of sizeof(mfa_set_state) (the staging buffer is 16-byte aligned whatever
// `states` is)
int mfa_match_batch_resume_set_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, mfa_set_state* states, uint8_t* results,
                                    int device) {
    if (!img || !offsets || !states) return MFA_ERR_INVALID_ARG;
    if (img->host.h.kind != MFA_KIND_NFA || !img->host.set_walk || img->host.set_wave) return MFA_ERR_UNSUPPORTED;
    return match_host_staged(bytes, offsets, n, results, device, [&](const uint8_t* d_bytes, const uint64_t* d_off, uint8_t* d_res, uint64_t, void* d_st) {
        return mfa_match_batch_resume_set(img, d_bytes, d_off, n, (mfa_set_state*)d_st, d_res, device, nullptr); }, states, sizeof(mfa_set_state), false);
}

static_assert(sizeof(mfa_set_state_wide) == 272 && offsetof(mfa_set_state_wide, nodes) == 16, "a wide record is seventeen 16-byte quarters: tag and reserved, then nodes[64], lane l's word at nodes[l]");

// which of the memory-less images the wide call takes: MFA_OK for a wave image, else the refusal
static int wide_takes(const mfa_image_t* img) {
    if (img->host.h.kind != MFA_KIND_NFA) return MFA_ERR_UNSUPPORTED;      // a memory automaton's state holds spans of the input: nothing to hand over
    if (!img->host.set_walk) return MFA_ERR_UNSUPPORTED;                   // a tabulated image's state is one number: mfa_match_batch_resume
    if (!img->host.set_wave) return MFA_ERR_UNSUPPORTED;                   // a lane image's set takes eight words: mfa_match_batch_resume_set
    return MFA_OK;
}

int mfa_match_batch_resume_set_wide(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, mfa_set_state_wide* d_states,
                                    uint8_t* d_results, int device, void* stream) {
    if (!img || !d_offsets || !d_states) return MFA_ERR_INVALID_ARG;
    int rc = wide_takes(img);
    if (rc != MFA_OK) return rc;
    if ((uintptr_t)d_states & 15u) return MFA_ERR_INVALID_ARG;             // the kernel reads and writes a record's tag as one 16-byte quarter
    if (n == 0) return MFA_OK;
    Launch L;
    if ((rc = launch_open(img, device, stream, MFA_KERNEL_NODESET, L)) != MFA_OK) return rc;
    if (const char* vb = getenv("MFA_VERBOSE"))      // (as mfa_match_batch: which kernel walks, on stderr)
        if (vb[0] == '1') fprintf(stderr, "mfa_hip: set walk of the automaton's nodes on strings in pieces, one string per wave (nfa_set_wave_resume_kernel)\n");
    return launch_nfa_set_wave_resume(img->host, *L.ds, *L.cx, d_bytes, d_offsets, n, reinterpret_cast<uint32_t*>(d_states), d_results, stream);
}

// host pointers: as mfa_match_batch_resume_set_host, with records of sizeof(mfa_set_state_wide)
int mfa_match_batch_resume_set_wide_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, mfa_set_state_wide* states, uint8_t* results,
                                         int device) {
    if (!img || !offsets || !states) return MFA_ERR_INVALID_ARG;
    const int rc = wide_takes(img);
    if (rc != MFA_OK) return rc;
    return match_host_staged(bytes, offsets, n, results, device, [&](const uint8_t* d_bytes, const uint64_t* d_off, uint8_t* d_res, uint64_t, void* d_st) {
        return mfa_match_batch_resume_set_wide(img, d_bytes, d_off, n, (mfa_set_state_wide*)d_st, d_res, device, nullptr); }, states, sizeof(mfa_set_state_wide), false);
}

int mfa_image_resume_state_bytes(mfa_image_t* img, uint32_t* bytes) {
    if (!img || !bytes) return MFA_ERR_INVALID_ARG;
    const HostImage& h = img->host;
    *bytes = h.h.kind != MFA_KIND_NFA ? 0u : !h.set_walk ? (uint32_t)sizeof(uint32_t) : h.set_wave ? (uint32_t)sizeof(mfa_set_state_wide) : (uint32_t)sizeof(mfa_set_state);
    return MFA_OK;
}

// ---- search inside lines (search.hip) ----------------------------------------------------------------------------------------------------
// which images the search takes: MFA_OK, or the refusal.  Builds the two tables on the way (search_tables.h), once per image; the caller
// holds img->mu
static int search_takes(mfa_image_t* img) {
    const HostImage& h = img->host;
    if (h.h.kind != MFA_KIND_NFA) return MFA_ERR_UNSUPPORTED;              // a memory automaton's step is no table walk
    if (h.set_walk || h.dfa_states > kSearchMaxSets) return MFA_ERR_UNSUPPORTED;      // no table, or one that no LDS holds
    if (img->search.rc == 1) (void)search_tables_build(h, img->search);
    return img->search.rc;                                                 // MFA_ERR_UNSUPPORTED: one of the two tables passed the limit
}

int mfa_image_search_info(mfa_image_t* img, uint32_t* pass1_states, uint32_t* pass2_states) {
    if (!img) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(img->mu);
    const int rc = search_takes(img);
    if (rc != MFA_OK) return rc;
    if (pass1_states) *pass1_states = img->search.pass1.states;
    if (pass2_states) *pass2_states = img->search.pass2.states;
    return MFA_OK;
}

int mfa_search_batch(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint8_t* d_results, uint64_t* d_spans,
                     uint8_t* d_span_results, int device, void* stream) {
    if (!img || !d_offsets || !d_results) return MFA_ERR_INVALID_ARG;
    if ((d_span_results && !d_spans) || ((uintptr_t)d_spans & 7u)) return MFA_ERR_INVALID_ARG;
    Launch L;
    L.lk = std::unique_lock<std::mutex>(img->mu);
    int rc = search_takes(img);
    if (rc != MFA_OK) return rc;
    if (n == 0) {
        if (!d_spans) return MFA_OK;
        if ((rc = check_device(device)) != MFA_OK) return rc;
        HIP_TRY(hipMemcpyAsync(d_spans, d_offsets, sizeof(uint64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));      // spans[0] = offsets[0]
        return MFA_OK;
    }
    if ((rc = device_prepare(img, device, &L.ds)) != MFA_OK) return rc;
    if ((rc = search_upload(img->search, *L.ds)) != MFA_OK) return rc;      // (the first call on this device: an allocation and a blocking copy)
    if ((rc = launch_open(img, device, stream, MFA_KERNEL_SEARCH, L)) != MFA_OK) return rc;
    return launch_search(img->host, img->search, *L.ds, *L.cx, d_bytes, d_offsets, n, d_results, d_spans, d_span_results, stream);
}

// host pointers: the staging of mfa_match_batch_host, with the spans (made absolute in the caller's offsets again) and their result bytes
int mfa_search_batch_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results, uint64_t* spans,
                          uint8_t* span_results, int device) {
    if (!img || !offsets || !results || (span_results && !spans)) return MFA_ERR_INVALID_ARG;
    {
        std::lock_guard<std::mutex> lk(img->mu);
        const int rc = search_takes(img);
        if (rc != MFA_OK) return rc;
    }
    if (n == 0) {
        if (spans) std::memcpy(spans, offsets, sizeof(uint64_t));
        return MFA_OK;
    }
    return match_host_staged(bytes, offsets, n, results, device, [&](const uint8_t* d_bytes, const uint64_t* d_off, uint8_t* d_res, uint64_t, void*) {
        uint64_t* d_spans = nullptr; uint8_t* d_sr = nullptr;
        int rc = MFA_OK;
        hipError_t e = spans ? hipMalloc((void**)&d_spans, (2u * n + 1u) * sizeof(uint64_t)) : hipSuccess;
        if (e == hipSuccess && span_results) e = hipMalloc((void**)&d_sr, 2u * n);
        if (e != hipSuccess) { set_last_hip_error((int)e); rc = MFA_ERR_HIP; }
        if (rc == MFA_OK) rc = mfa_search_batch(img, d_bytes, d_off, n, d_res, d_spans, d_sr, device, nullptr);
        if (rc == MFA_OK) {
            std::vector<uint64_t> sp(spans ? 2u * n + 1u : 0u);
            e = hipDeviceSynchronize();
            if (e == hipSuccess && spans) e = hipMemcpy(sp.data(), d_spans, sp.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
            if (e == hipSuccess && span_results) e = hipMemcpy(span_results, d_sr, 2u * n, hipMemcpyDeviceToHost);
            if (e != hipSuccess) { set_last_hip_error((int)e); rc = MFA_ERR_HIP; }
            for (uint64_t& x : sp) x += offsets[0];
            if (rc == MFA_OK && spans) std::memcpy(spans, sp.data(), sp.size() * sizeof(uint64_t));
        }
        if (d_spans) (void)hipFree(d_spans);
        if (d_sr) (void)hipFree(d_sr);
        return rc;
    });
}

int mfa_last_kernel_ms(mfa_image_t* img, int device, float* ms) {
    if (!img || !ms) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(img->mu);
    LaunchCtx* cx = last_ctx(img, device);
    if (!cx) return MFA_ERR_INVALID_ARG;
    HIP_TRY(hipEventSynchronize((hipEvent_t)cx->ev_stop));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)cx->ev_start, (hipEvent_t)cx->ev_stop));
    jit_print_stats(*cx, "last kernel");
    return MFA_OK;
}

int mfa_last_dfa_split(mfa_image_t* img, int device, uint64_t* strings, uint64_t* chunks, uint32_t* chunk_bytes) {
    uint32_t h[SPLIT_H_WORDS] = {0};
    const int rc = last_split_header(img, device, &LaunchCtx::split_ran, h);
    if (rc != MFA_OK) return rc;
    split_words(h, strings, chunks, chunk_bytes);
    return MFA_OK;
}

int mfa_last_dfa_spec(mfa_image_t* img, int device, uint64_t* rewalked_chunks, uint64_t* serial_strings, uint64_t* serial_bytes) {
    uint32_t h[SPLIT_H_WORDS] = {0};
    const int rc = last_split_header(img, device, &LaunchCtx::spec_ran, h);
    if (rc != MFA_OK) return rc;
    spec_words(h, rewalked_chunks, serial_strings, serial_bytes);
    return MFA_OK;
}

int mfa_last_set_split(mfa_image_t* img, int device, uint64_t* strings, uint64_t* chunks, uint32_t* chunk_bytes, uint64_t* rewalked_chunks,
                       uint64_t* serial_strings, uint64_t* serial_bytes) {
    uint32_t h[SPLIT_H_WORDS] = {0};
    const int rc = last_split_header(img, device, &LaunchCtx::set_split_ran, h);
    if (rc != MFA_OK) return rc;
    split_words(h, strings, chunks, chunk_bytes);
    spec_words(h, rewalked_chunks, serial_strings, serial_bytes);
    return MFA_OK;
}

int mfa_last_region_ms(mfa_image_t* img, int device, float* ms) {
    if (!img || !ms) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(img->mu);
    LaunchCtx* cx = last_ctx(img, device);
    if (!cx) return MFA_ERR_INVALID_ARG;
    *ms = 0.0f;
    if (!cx->ran_regions) return MFA_OK;
    HIP_TRY(hipEventSynchronize((hipEvent_t)cx->ev_r1));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)cx->ev_r0, (hipEvent_t)cx->ev_r1));
    return MFA_OK;
}

int mfa_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return MFA_ERR_NO_DEVICE;
    return count;
}

int mfa_last_hip_error(void) { return g_last_hip_error; }

const char* mfa_strerror(int code) {
    switch (code) {
        case MFA_OK: return "ok";
        case MFA_ERR_INVALID_ARG: return "invalid argument";
        case MFA_ERR_BAD_BLOB: return "malformed automaton image blob";
        case MFA_ERR_UNSUPPORTED: return "automaton outside the limits of the device kernels";
        case MFA_ERR_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
        case MFA_ERR_HIP: return "HIP runtime error";
        case MFA_ERR_NOMEM: return "out of host memory";
        case MFA_ERR_TOO_LONG: return "string longer than MFA_MAX_STRING_BYTES";
        case MFA_ERR_JIT: return "compiling the specialised kernel failed";
    }
    return "unknown error";
}

const char* mfa_version(void) { return "mfa_hip 0.1 (gfx950)"; }

}  // extern "C"
