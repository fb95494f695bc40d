// api.hip -- the extern "C" boundary declared in include/stringwars_amd.h.
//
// Host-side plumbing only: scope/engine lifetime, residency detection and staging of host tapes,
// scratch carving, the device pre-pass, kernel dispatch and optional hipEvent timing. There is no
// CPU compute path in this library: without a HIP device every entry point fails with
// swh_no_device_k.
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "common.hpp"
#include "within.hpp"
#include "align.hpp"
#include "infix.hpp"
#include "osa.hpp"
#include "lcs.hpp"
#include "jaro.hpp"
#include "extract.hpp"
#include <algorithm>
#include <mutex>
#include <utility>

namespace swh {

// ---- error text (static storage, one slot per thread) ----------------------------------------
static thread_local char g_error_text[512];
__attribute__((format(printf, 3, 4))) static swh_status_t fail(const char **error, swh_status_t status, const char *fmt, ...) {
    va_list args;
    va_start(args, fmt);
    vsnprintf(g_error_text, sizeof g_error_text, fmt, args);
    va_end(args);
    if (error) *error = g_error_text;
    return status;
}
static swh_status_t fail_hip(const char **error, const HipFailure &f) {
    (void)hipGetLastError();
    return fail(error, f.code == hipErrorOutOfMemory ? swh_bad_alloc_k : swh_device_error_k, "HIP error '%s' in %s", hipGetErrorString(f.code), f.what);
}

// ---- kernel stamps -------------------------------------------------------------------------------
// STRINGWARS_AMD_TRACE=1: every stamped launch is announced on stderr and waited for -- the last name printed before a device
// fault is the kernel behind it (diagnostics only: it serialises everything).
static bool trace_launches() {
    static const bool on = [] { const char *e = getenv("STRINGWARS_AMD_TRACE"); return e && atoi(e) != 0; }();
    return on;
}
// STRINGWARS_AMD_STAMPS=1: with profiling on, the start and the length of every stamped launch of a call (event times) on stderr.
static bool trace_stamps() {
    static const bool on = [] { const char *e = getenv("STRINGWARS_AMD_STAMPS"); return e && atoi(e) != 0; }();
    return on;
}
StampGuard::StampGuard(Scope *s, const char *name) : scope(s), idx(0), on(s->profiling) {
    if (trace_launches()) { fprintf(stderr, "[swh] launch %s\n", name); fflush(stderr); }
    if (!on) return;
    if (scope->stamps_used == scope->stamps.size()) {
        KernelStamp st{};
        if (hipEventCreate(&st.start) != hipSuccess || hipEventCreate(&st.stop) != hipSuccess) { on = false; return; }
        scope->stamps.push_back(st);
    }
    idx = scope->stamps_used++;
    scope->stamps[idx].name = name;
    (void)hipEventRecord(scope->stamps[idx].start, scope->stream);
}
StampGuard::~StampGuard() {
    if (on) (void)hipEventRecord(scope->stamps[idx].stop, scope->stream);
    if (trace_launches()) {
        const hipError_t err = hipStreamSynchronize(scope->stream);
        fprintf(stderr, "[swh]   done (%s)\n", hipGetErrorString(err)); fflush(stderr);
    }
}

static void collect_timing(Scope *scope) {
    swh_timing_t &t = scope->last_timing;
    t.total_ms = 0; t.dominant_ms = 0; t.compute_ms = 0; t.dominant_name[0] = 0; t.kernels = (uint32_t)scope->stamps_used;
    if (!scope->stamps_used) return;
    float span = 0;
    for (size_t i = 0; i < scope->stamps_used; ++i) {   // the last kernel to finish need not be the last one launched
        float to_stop = 0;
        (void)hipEventElapsedTime(&to_stop, scope->stamps[0].start, scope->stamps[i].stop);
        if (to_stop > span) span = to_stop;
    }
    t.total_ms = span;
    // DP kernels may run side by side on two streams (wavefront classes): compute_ms is the length of the UNION of
    // their intervals, not the sum of their durations
    std::vector<std::pair<float, float>> dp;
    for (size_t i = 0; i < scope->stamps_used; ++i) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, scope->stamps[i].start, scope->stamps[i].stop);
        if (strncmp(scope->stamps[i].name, "plan_", 5) != 0 && strncmp(scope->stamps[i].name, "utf8_", 5) != 0) {
            float from = 0;
            (void)hipEventElapsedTime(&from, scope->stamps[0].start, scope->stamps[i].start);
            dp.emplace_back(from, from + ms);
        }
        if (trace_launches() || trace_stamps()) {
            float from = 0;
            (void)hipEventElapsedTime(&from, scope->stamps[0].start, scope->stamps[i].start);
            fprintf(stderr, "[swh] stamp %-28s start %8.3f ms  length %8.3f ms\n", scope->stamps[i].name, from, ms);
        }
        if (ms > t.dominant_ms) {
            t.dominant_ms = ms;
            snprintf(t.dominant_name, sizeof t.dominant_name, "%s", scope->stamps[i].name);
        }
    }
    std::sort(dp.begin(), dp.end());
    float covered = 0, reach = -1e30f;
    for (const auto &iv : dp) {
        if (iv.first > reach) { covered += iv.second - iv.first; reach = iv.second; }
        else if (iv.second > reach) { covered += iv.second - reach; reach = iv.second; }
    }
    t.compute_ms = covered;
}

static void add_to_totals(swh_timing_totals_t &totals, const swh_timing_t &call) {
    totals.total_ms += call.total_ms;
    totals.dominant_ms += call.dominant_ms;
    totals.compute_ms += call.compute_ms;
    totals.calls += 1;
}

// Reads the events of the scope's last call once they are complete and adds the call to the running totals.
// `complete`: the caller has synchronised with the scope's last call. Otherwise (the start of the next call in
// asynchronous mode) completion is only known when profiling is on, through the call's stop events.
static void harvest_timing(Scope *scope, bool complete) {
    const bool timed = scope->profiling && scope->stamps_pending && scope->stamps_used;
    if (timed) {
        for (size_t i = 0; i < scope->stamps_used; ++i) (void)hipEventSynchronize(scope->stamps[i].stop);   // two streams: no single last event
        complete = true;
    }
    const uint64_t cells = scope->last_timing.cells, bytes = scope->last_timing.bytes;
    if (timed) {
        collect_timing(scope);
        scope->last_timing.cells = cells; scope->last_timing.bytes = bytes;
    }
    // a plan-free call reports its work units through host-mapped memory
    if (scope->summary_pending && complete) {
        const CallSummary sm = scope->summary_host[scope->summary_slot];
        scope->last_timing.cells = sm.cells;
        scope->last_timing.bytes = (scope->summary_extra_bytes ? scope->summary_extra_bytes : sm.symbols * scope->summary_sym_bytes) +
                                   scope->summary_pairs * (2 * scope->summary_ow + scope->summary_elem);
        if (!sm.violation) {
            scope->hint_lengths = true;
            scope->hint_max_la = sm.max_la; scope->hint_max_lb = sm.max_lb;
            scope->hint_mean_x16 = scope->summary_pairs ? (uint32_t)std::min<uint64_t>(sm.symbols * 8 / scope->summary_pairs, 0xFFFFFFu) : 0u;
            scope->hint_mean_string_x16 = scope->summary_strings ? (uint32_t)std::min<uint64_t>(sm.symbols * 16 / scope->summary_strings, 0xFFFFFFu) : 0u;
            scope->hint_short = (uint64_t)sm.short_pairs * 4 >= scope->summary_pairs;
        } else if (scope->async) {
            // An asynchronous plan-free call cannot be redone behind the caller's back (synchronous calls are: run_call_on).
            // It only runs on prepared tapes, whose lengths were measured: a pair that does not fit means the tape's memory
            // changed after swh_tape_prepare_* -- the misfit pairs were NOT scored. Reported by the next synchronisation.
            scope->violation_seen = true;
        }
    }
    scope->summary_pending = false;
    if (timed) add_to_totals(scope->totals, scope->last_timing);
    scope->stamps_pending = false;
}

// ---- scratch -------------------------------------------------------------------------------------
static size_t pad(size_t n) { return (n + 255) & ~(size_t)255; }
struct Carver {
    char *base; size_t used, cap;
    template <typename T> T *take(size_t n) {
        char *p = base ? base + used : nullptr;
        used += pad(n * sizeof(T));
        return (T *)p;
    }
};

static void ensure(char *&buf, size_t &cap, size_t need) {
    if (need <= cap) return;
    if (buf) SWH_HIP_CHECK(hipFree(buf));
    buf = nullptr; cap = 0;
    size_t want = need + need / 4 + (1 << 20);
    SWH_HIP_CHECK(hipMalloc((void **)&buf, want));
    cap = want;
}

// both tapes of a call up to this size (together) are staged by one launch pair; STRINGWARS_AMD_UTF8_MERGED_MB=n moves it
static uint64_t utf8_merged_bytes() {
    static const uint64_t bytes = [] { const char *e = test_hook("STRINGWARS_AMD_UTF8_MERGED_MB"); return e ? (uint64_t)atol(e) << 20 : ~0ull; }();
    return bytes;
}
// STRINGWARS_AMD_UTF8_STAGING: `strings` -- every raw UTF-8 call on the planned / tiled routes stages string by string (k_utf8_strings: the
// tests send words and empty strings through it), `tiles` -- never (the flat one-pass kernel: the comparison), unset -- tapes whose
// mean string has at least kUtf8StringsMeanBytes bytes.
static int utf8_strings_mode() {
    static const int mode = [] { const char *e = test_hook("STRINGWARS_AMD_UTF8_STAGING"); return !e ? 0 : (!strcmp(e, "strings") ? 1 : (!strcmp(e, "tiles") ? 2 : 0)); }();
    return mode;
}
// u32 words of scratch the flat UTF-8 decoder needs for a tape of `bytes` bytes (see launch_utf8_decode)
static size_t utf8_scratch_words(uint64_t bytes) {
    // mirrors the carving in launch_utf8_decode: tile counts | sub-tile prefixes | u64 tile prefixes | u64 block sums | balances
    // (the look-back words and tickets of the one-pass kernel live in scope->utf8_status / the call's flag words)
    uint64_t tiles = (bytes + kUtf8Tile - 1) / kUtf8Tile;
    return (size_t)((tiles + 4) + (kUtf8Subs * tiles + 4) + 2 * (tiles + 4) + 2 * ((tiles + 1023) / 1024 + 4) + (tiles + 6));
}

static bool is_device_pointer(const void *p) {
    if (!p) return true;
    hipPointerAttribute_t attr;
    hipError_t err = hipPointerGetAttributes(&attr, p);
    if (err != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// hipMalloc'ed memory of a device (not managed, not host-mapped): where a write-through store that was acknowledged can be read by anybody
// -- ON THE SCOPE'S OWN DEVICE: agent-scope write-through is visibility on that agent; a peer device's memory takes the stream's way
static bool is_plain_device_memory(const void *p, int device) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t err = hipPointerGetAttributes(&attr, p);
    if (err != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice && attr.device == device;
}

// ---- one engine call ---------------------------------------------------------------------------
struct HostTape { const uint8_t *data; const void *offsets; size_t count; int off64; };

// swh_prepared_t: a tape made ready once -- resident on the device, measured, and (UTF-8) validated and decoded --
// the counterpart of the `BytesTapeView` / `CharsTapeView` the reference builds ONCE outside its timed closures
// (bench.rs:292-306) and sub-views per iteration (bench.rs:134-139).
struct Prepared {
    int device = 0;
    bool utf8 = false;           // symbols are Unicode scalar values
    bool ascii = false;          // utf8 and every code point is one byte: the byte tape is the code-point tape
    uint32_t off64 = 0;          // width of the byte tape's offsets
    TapeRef bytes{};             // device: u8 data, u32/u64 offsets
    TapeRef symbols{};           // utf8: u32 code points + u64 code-point offsets; otherwise unused
    uint64_t total_bytes = 0, total_symbols = 0;   // offsets[count]: the end of the last string (and, of the symbols, how many were decoded)
    uint64_t first_byte = 0;     // offsets[0]: a tape may be a window of a larger buffer
    uint32_t longest_bytes = 0, longest_symbols = 0;
    std::vector<void *> owned;   // device buffers that go with the handle
};

struct CallSpec {
    HostTape a, b;
    bool cross, utf8;
    uint32_t bound;
    void *out; size_t out_stride, row_stride; bool out64;
    const Prepared *pa = nullptr, *pb = nullptr;   // prepared tapes (both or neither); a.count / b.count = the views' counts
    size_t a_first = 0, b_first = 0;
    bool force_planned = false;                    // redo of a call whose plan-free kernel met a pair it could not score
    uint32_t skip_upto = 0;                        // ... where that kernel HAS scored every pair of two strings of at most this many symbols
    bool flat_staging = false;                     // redo of a raw UTF-8 call whose string-by-string staging met a string too long for it
};

// ---- prepared tapes in a call -------------------------------------------------------------------------------------------------
static bool view_fits(const swh_prepared_view_t *view) {
    const Prepared *p = (const Prepared *)view->tape;
    return view->first <= p->bytes.count && view->count <= p->bytes.count - view->first;
}
static swh_status_t check_prepared_pair(const Scope *scope, const Prepared *pa, const Prepared *pb, const char **error) {
    if (pa->utf8 != pb->utf8) return fail(error, swh_invalid_argument_k, "one tape was prepared as UTF-8, the other as bytes");
    if (pa->device != scope->device || pb->device != scope->device)
        return fail(error, swh_invalid_argument_k, "a prepared tape lives on another device than the scope");
    return swh_success_k;
}
// strings [first, first + count) of a prepared tape: its code points (`code_points` on a UTF-8 tape: u64 offsets) or its bytes
static TapeRef prepared_view(const Prepared *p, bool code_points, size_t first, size_t count) {
    const bool decoded = code_points && p->utf8;
    TapeRef t = decoded ? p->symbols : p->bytes;
    t.offsets = (const char *)t.offsets + first * (decoded || p->off64 ? 8 : 4);
    t.count = count;
    return t;
}

static uint64_t read_offset(const void *offs, int off64, size_t i, bool device, hipStream_t stream) {
    uint64_t v = 0;
    size_t w = off64 ? 8 : 4;
    if (device) {
        SWH_HIP_CHECK(hipMemcpyAsync(&v, (const char *)offs + i * w, w, hipMemcpyDeviceToHost, stream));
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
    } else {
        memcpy(&v, (const char *)offs + i * w, w);
    }
    return v;
}

static swh_status_t run_call_on(Scope *scope, const Engine *engine, const CallSpec &spec, const char **error);

// Does either tape hold a byte above 0x7F? Runs in front of the byte kernels when a UTF-8 call BELIEVES its raw tapes to be ASCII
// (they were, the last time this scope staged them): sixteen bytes per thread and step, the flag in host-mapped memory.
// The tapes' byte totals are read HERE, from offsets[count]: the caller's belief about them may be as stale as the one about their bytes.
__global__ __launch_bounds__(256) void k_ascii_check(const uint8_t *a, const void *a_offsets, uint64_t a_count, const uint8_t *b, const void *b_offsets,
                                                     uint64_t b_count, uint32_t off64, uint32_t *flag) {
    uint32_t high = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256 * 16;
    for (int t = 0; t < 2; ++t) {
        const uint8_t *data = t ? b : a;
        const void *offsets = t ? b_offsets : a_offsets;
        if (!offsets) continue;
        const uint64_t count = t ? b_count : a_count;
        const uint64_t bytes = off64 ? ((const uint64_t *)offsets)[count] : (uint64_t)((const uint32_t *)offsets)[count];
        for (uint64_t at = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16; at < bytes; at += stride) {
            if (at + 16 <= bytes) {
                uint4 v;
                __builtin_memcpy(&v, data + at, 16);
                high |= v.x | v.y | v.z | v.w;
            } else {
                for (uint64_t i = at; i < bytes; ++i) high |= data[i];
            }
        }
    }
    if (__ballot((high & 0x80808080u) != 0) != 0 && (threadIdx.x & 63) == 0) __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

static swh_status_t run_call(Scope *scope, const Engine *engine, const CallSpec &spec, const char **error) {
    if (!scope || !engine) return fail(error, swh_invalid_argument_k, "null scope or engine");
    if (!scope->pipelined) return run_call_on(scope, engine, spec, error);
    Scope *lane = scope->lanes[scope->next_lane];
    scope->next_lane ^= 1;
    scope->last_lane = lane;
    // The lane starts where the caller's stream is now: whatever was enqueued there before this call -- the producer of
    // the inputs, or a consumer still reading the output buffer this call is about to overwrite (an RCCL gather of an
    // earlier step) -- completes first. swh_scope_join gives the other direction.
    if (hipEventRecord(scope->order_ev, scope->stream) != hipSuccess ||
        hipStreamWaitEvent(lane->stream, scope->order_ev, 0) != hipSuccess)
        return fail(error, swh_device_error_k, "could not order a pipeline lane after the scope's stream");
    swh_status_t status = run_call_on(lane, engine, spec, error);
    if (status == swh_success_k && hipEventRecord(lane->lane_done, lane->stream) != hipSuccess)
        return fail(error, swh_device_error_k, "hipEventRecord failed on a pipeline lane");
    scope->last_timing = lane->last_timing;
    return status;
}

// Which kernels a unit-cost Levenshtein call runs on.
enum Route { kRoutePlanned, kRouteTiled, kRouteDirectShort, kRouteShortTiled, kRouteCrossShort, kRouteAlignShort, kRouteAlignLong };

// Strings up to this many symbols (G <= 8 blocks) are scored by the tiled kernel when their lengths are known; beyond it
// a tile holds too few pairs per block count and the global sort of the planned path packs the waves better.
static uint32_t tiled_longest_limit() {
    static const uint32_t limit = [] { const char *e = test_hook("STRINGWARS_AMD_TILED_MAX"); return e ? (uint32_t)atoi(e) : 256u; }();
    return limit;
}
// Word-sized batches: k_short_tiled (<= 16 bytes, batches large enough to give every workgroup a chunk worth sorting) /
// k_direct_short (<= 32 bytes, small batches). Comparison knob STRINGWARS_AMD_SHORT: `direct`
// keeps k_direct_short for all of them, `tiled` sends them to the general tiled kernel.
// (STRINGWARS_AMD_SHORT_MIN_PAIRS, read per call: the tests send small batches to the chunked kernel with it)
static uint64_t short_tiled_min_pairs() {
#ifdef SWH_TEST_HOOKS
    const char *e = test_hook("STRINGWARS_AMD_SHORT_MIN_PAIRS");   // (the test library reads it per call: the tests move it between calls)
    return e ? (uint64_t)atoll(e) : (uint64_t)1 << 16;
#else
    static const uint64_t pairs = [] { const char *e = test_hook("STRINGWARS_AMD_SHORT_MIN_PAIRS"); return e ? (uint64_t)atoll(e) : (uint64_t)1 << 16; }();
    return pairs;
#endif
}
// Bounds up to here may take the banded kernel (STRINGWARS_AMD_BAND_MAX=63: the one-word windows only, the comparison knob).
static uint32_t band_max_bound() {
    static const uint32_t most = [] { const char *e = test_hook("STRINGWARS_AMD_BAND_MAX"); const uint32_t v = e ? (uint32_t)atoi(e) : kBandMaxBound; return v > kBandMaxBound ? kBandMaxBound : v; }();
    return most;
}
// Longest string k_align_cross_long is chosen for: the longest query it takes (STRINGWARS_AMD_ALIGN_LONG_MAX=n lowers it) ...
static uint32_t align_long_limit() {
    static const uint32_t limit = [] { const char *e = test_hook("STRINGWARS_AMD_ALIGN_LONG_MAX"); const uint32_t v = e ? (uint32_t)atoi(e) : 4096u; return v > 4096u ? 4096u : v; }();
    return limit;
}
// ... and per form, the length up to which it measured faster than the column-profile kernel on DNA cross-products (TCUPS, long
// kernel : profile kernel):       1 K symbols        3 K symbols
//      NW linear  (W = 128)       12.8 :  9.9        12.6 : 10.5       -> as far as the kernel goes (a boundary buffer of 2.2 GB there)
//      NW affine  (W =  64)        6.1 :  5.7         5.8 :  6.1       -> 2048
//      SW linear  (W =  64)        6.9 :  6.1         6.6 :  6.6       -> 2048
//      SW affine  (W =  32)        3.7 :  3.7         3.9 :  3.9       -> stays where the wavefront class kernels were the alternative
static uint32_t align_long_pays(bool local, bool affine) { return local && affine ? 384u : (local || affine ? 2048u : 4096u); }
// A synchronous call whose results stay on the device returns when its summary has LANDED -- the last workgroup writes that word
// into host-mapped memory once every workgroup's (write-through) result stores were acknowledged -- instead of when the stream
// reports the kernel complete: the end of a kernel as the runtime sees it (the release that writes the L2s back, the completion
// signal, the wake-up) costs ~5 us that no result waits for (tools/launch_probe.hip: 12.5 us against 7.3 for an empty kernel).
// What the stream still orders is unchanged: the scope's next call, its copies, swh_scope_synchronize. Only for outputs in plain
// device memory (hipMalloc), outside profiling, on the routes whose one kernel reports the summary; after 2 ms of polling the
// call waits for the stream the ordinary way. STRINGWARS_AMD_EARLY_RETURN=0 always does.
static bool early_return_on() {
    static const bool on = [] { const char *e = getenv("STRINGWARS_AMD_EARLY_RETURN"); return !e || atoi(e) != 0; }();
    return on;
}
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    asm volatile("" ::: "memory");
#endif
}
// The poll is bounded by what the scope's previous early-returning call took: a call that ran for more than ~0.4 ms last time waits for
// the stream straight away (5 us are nothing to it, and a core spinning for milliseconds per call is), a shorter one spins for at most
// four times that -- never more than 2 ms -- before it falls back to the stream (which also reports a kernel that died).
static void wait_for_summary(Scope *scope, hipStream_t stream) {
    volatile uint32_t *landed = &scope->summary_host[0].landed;
    const auto begun = std::chrono::steady_clock::now();
    const auto finish = [&]() {
        const auto took = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - begun).count();
        scope->early_return_last_us = (uint32_t)std::min<long long>(took, 1000000);
    };
    if (scope->early_return_last_us > 400) {
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        finish();
        return;
    }
    const auto patience = std::chrono::microseconds(std::min<uint32_t>(2000u, std::max<uint32_t>(100u, 4u * scope->early_return_last_us)));
    for (uint32_t spins = 1;; ++spins) {
        if (__atomic_load_n(landed, __ATOMIC_ACQUIRE)) { finish(); return; }
        if ((spins & 0xFFu) == 0 && std::chrono::steady_clock::now() - begun > patience) {
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            finish();
            return;
        }
        cpu_relax();
    }
}

static int short_route_choice() {
    static const int choice = [] {
        const char *e = test_hook("STRINGWARS_AMD_SHORT");
        return !e ? 0 : (!strcmp(e, "direct") ? 1 : (!strcmp(e, "tiled") ? 2 : 0));
    }();
    return choice;
}

static bool bitparallel_ok(const Engine *engine) {
    return engine->kind == 0 && engine->unit_costs && engine->algorithm != swh_algorithm_wavefront_k;
}
static uint64_t call_pairs(const CallSpec &spec) { return spec.cross ? (uint64_t)spec.a.count * spec.b.count : spec.a.count; }

// What a call knows about its strings' lengths before it launches anything: a guarantee for prepared tapes, a belief from the scope's
// previous call (the kernels verify it), or -- a Levenshtein engine forced onto the tiled kernel -- that kernel's 2048 symbols.
struct Lengths {
    bool known = false, guaranteed = false;
    uint32_t la_max = 0, lb_max = 0;
    uint64_t prepared_mean_x16 = 0;   // prepared tapes: the longer mean string of the two whole tapes, bytes x 16
};
static Lengths call_lengths(const Scope *scope, const Engine *engine, const CallSpec &spec, bool utf8) {
    Lengths l;
    if (spec.pa) {
        l.known = l.guaranteed = true;
        l.la_max = utf8 ? spec.pa->longest_symbols : spec.pa->longest_bytes;
        l.lb_max = utf8 ? spec.pb->longest_symbols : spec.pb->longest_bytes;
        const uint64_t ma = spec.pa->bytes.count ? (spec.pa->total_bytes - spec.pa->first_byte) * 16 / spec.pa->bytes.count : 0;
        const uint64_t mb = spec.pb->bytes.count ? (spec.pb->total_bytes - spec.pb->first_byte) * 16 / spec.pb->bytes.count : 0;
        l.prepared_mean_x16 = std::max(ma, mb);   // (of the WHOLE tapes, whatever the view: a view's own bytes would cost a read of its two offsets per call)
    } else if (scope->hint_lengths) {
        l.known = true;
        l.la_max = scope->hint_max_la; l.lb_max = scope->hint_max_lb;
    } else if (engine->kind == 0 && engine->algorithm == swh_algorithm_tiled_k) {
        l.known = true;
        l.la_max = l.lb_max = 2048;
    }
    return l;
}

struct RouteChoice {
    Route route = kRoutePlanned;
    uint32_t longest = 0;      // what the plan-free kernel is launched for
    bool align_wide = false;   // kRouteAlignShort on k_align_cross_wide (its alphabet condition is checked by the kernel)
};
// Which kernels a call runs on (DESIGN.md §4's route table). Calls no HIP API and changes nothing on the scope. `dev_out`: the output is
// in device memory, where an asynchronous call cannot look at the outcome -- it only acts on lengths that are guaranteed.
static RouteChoice pick_route(const Scope *scope, const Engine *engine, const CallSpec &spec, bool utf8, bool dev_out, const Lengths &len) {
    RouteChoice r;
    const bool can_verify = !scope->async || !dev_out;
    const bool usable = len.known && (len.guaranteed || can_verify);
    const uint32_t both = std::max(len.la_max, len.lb_max);
    if (engine->kind == 0) {
        // Unit-cost Levenshtein whose string lengths are known skips the planning pre-pass altogether.
        if (!bitparallel_ok(engine) || spec.force_planned || engine->algorithm == swh_algorithm_bitparallel_k || !usable) return r;
        r.longest = both;
        // plan_key(): the banded kernel wins from ~6 blocks at k = 32 (bounds of 64 .. 255: where band_cost() says so)
        const bool band_pays = spec.bound <= 63 ? both > 32
                                                : spec.bound <= band_max_bound() && band_cost(spec.bound) < (utf8 ? 40u : 28u) * ((both + 31) >> 5);
        const int choice = short_route_choice();
        if (engine->algorithm == swh_algorithm_tiled_k)
            r.route = (!len.guaranteed || std::min(len.la_max, len.lb_max) <= 2048) ? kRouteTiled : kRoutePlanned;
        else if (!band_pays && both <= tiled_longest_limit()) {
            if (both <= 32 && choice != 2 && spec.cross) r.route = kRouteCrossShort;   // k_cross_short, or k_cross_short_cp for code points
            else if (both <= 32 && choice != 2 && !utf8)
                r.route = both <= 16 && call_pairs(spec) >= short_tiled_min_pairs() && choice == 0 ? kRouteShortTiled : kRouteDirectShort;
            else r.route = kRouteTiled;
        }
        return r;
    }
    // Alignment scores on a class table when both tapes hold word-sized strings only (the reference's default `words` token mode,
    // bench.rs:271): one pair per lane, no pre-pass (alignshort.hip). STRINGWARS_AMD_ALIGN_SHORT=0 keeps them on the planned path.
    static const bool align_short_on = [] { const char *e = test_hook("STRINGWARS_AMD_ALIGN_SHORT"); return !e || atoi(e) != 0; }();
    if (!engine->scoring.class_table || utf8 || spec.force_planned || !align_short_on) return r;
    // up to 128 symbols for cross-products with linear gaps, as long as the candidates of a work item use at most eight symbol
    // classes (DNA; the kernel checks per item, a scope that met richer text stops trying -- `align_wide_off`)
    static const bool wide_on = [] { const char *e = test_hook("STRINGWARS_AMD_ALIGN_WIDE"); return !e || atoi(e) != 0; }();   // comparison knob: 0 = the multi-pass kernel instead
    // (what the latch is keyed by: prepared handles, else the tapes' data pointers -- sub-views of one tape share them)
    const void *key_a = spec.pa ? (const void *)spec.pa : (const void *)spec.a.data, *key_b = spec.pb ? (const void *)spec.pb : (const void *)spec.b.data;
    const bool wide_off = scope->align_wide_off.engine == engine->uid && scope->align_wide_off.a == key_a && scope->align_wide_off.b == key_b;
    const bool affine = engine->scoring.open != engine->scoring.extend;
    const bool wide = wide_on && spec.cross && both <= 128 && !affine && !wide_off && can_verify;
    const uint32_t per_item = align_long_queries(scope, spec.a.count, spec.b.count);
    const uint64_t long_items = ((uint64_t)(spec.b.count + 63) / 64) * ((uint64_t)(spec.a.count + per_item - 1) / per_item);
    if (usable && (both <= 32 || wide)) {
        r.route = kRouteAlignShort;
        r.longest = both;
        r.align_wide = both > 32;
    } else if (len.known && can_verify && spec.cross && !wide_off && both <= std::min(align_long_limit(), align_long_pays(engine->kind == 2, affine)) &&
               align_long_fits(scope, long_items, len.la_max, affine)) {
        // longer ones on the same small-alphabet condition: columns in passes of 128 (local or Gotoh: 64, both: 32), the boundary
        // column between passes through global memory (alignshort.hip: k_align_cross_long), up to where it beats the
        // column-profile kernel (align_long_pays)
        r.route = kRouteAlignLong;
        r.longest = len.la_max;
    } else if (usable && both <= 64) {
        // tokens of up to 64 bytes over any alphabet (multilingual words: ~5 code points are ~11 bytes, their tail reaches past 32):
        // the lane-per-pair kernel with a register row of 64 cells
        r.route = kRouteAlignShort;
        r.longest = both;
    } else if (len.known && can_verify && !scope->async) {
        // word tokens with a FEW long ones among them (a URL, a sentence of a script that writes no spaces): the lane kernel scores
        // every pair of two strings that fit its 64 cells, reports that some did not, and the redo plans only the pairs with a
        // longer string (`skip_upto`) -- instead of 4 M word pairs on kernels built for long strings (2048 x 2048 multilingual
        // words with one token of 70 bytes: 2.2 ms per call, NW linear). Taken when the mean string is word-sized.
        const uint64_t mean_x16 = spec.pa ? len.prepared_mean_x16 : scope->hint_mean_string_x16;
        if (mean_x16 && mean_x16 <= 24 * 16) {
            r.route = kRouteAlignShort;
            r.longest = 64;
        }
    }
    return r;
}

// ---- one engine call, in phases ----------------------------------------------------------------------------------------------
// run_call_on checks the call, then runs attempts until one is done. An attempt that finds out that what it launched cannot stand
// (the tapes' totals changed, a string too long for the string-by-string staging, a length or alphabet belief that did not hold,
// a fused planner that could not gather its grid) updates the scope where it found out and hands back the spec of the next attempt.
static swh_status_t check_call(Scope *scope, const Engine *engine, const CallSpec &spec, const char **error) {
    if (!scope || !engine) return fail(error, swh_invalid_argument_k, "null scope or engine");
    if (!spec.out && spec.a.count) return fail(error, swh_invalid_argument_k, "null output pointer");
    if (!spec.cross && spec.a.count != spec.b.count)
        return fail(error, swh_invalid_argument_k, "pairwise call needs tapes of equal count");
    if (call_pairs(spec) >= 0xFFFFFFF0ull) return fail(error, swh_unsupported_length_k, "more than 2^32 pairs in one call");
    if (!spec.pa) return swh_success_k;
    if (!spec.pb) return fail(error, swh_invalid_argument_k, "both tapes must be prepared, or neither");
    return check_prepared_pair(scope, spec.pa, spec.pb, error);
}

static bool believe_sizes() {
    static const bool believe = [] { const char *e = test_hook("STRINGWARS_AMD_SIZE_BELIEF"); return !e || atoi(e) != 0; }();
    return believe;
}
static bool same_as_believed(const HostTape &t, const Scope::SizeBelief &slot) {
    return slot.valid && slot.data == t.data && slot.offsets == t.offsets && slot.count == t.count && slot.off64 == t.off64;
}
static void remember_total(Scope::SizeBelief &slot, const HostTape &t, uint64_t bytes, bool valid) {
    slot = Scope::SizeBelief{t.data, t.offsets, t.count, t.off64, bytes, valid, false};
}
// Does the allocation that holds `p` reach `bytes` beyond it? A belief about a raw device tape is only acted on where it does.
static bool allocation_covers(const void *p, uint64_t bytes) {
    void *base = nullptr; size_t size = 0;
    return hipMemGetAddressRange((hipDeviceptr_t *)&base, &size, (hipDeviceptr_t)p) == hipSuccess && (const char *)p + bytes <= (const char *)base + size;
}

constexpr uint32_t kDoublingBound = 63;
struct Doubling { bool on = false; double need = 0; };

// One attempt at a call: its state, filled phase by phase, and the phases. What follows from the spec alone comes first.
struct Call {
    Scope *scope; const Engine *engine; const CallSpec &spec; const char **error;
    hipStream_t stream = scope->stream;
    uint64_t pairs = call_pairs(spec);
    bool prepared = spec.pa != nullptr, bitpar_ok = bitparallel_ok(engine);
    // code points of pure-ASCII tapes are their bytes: such a pair of prepared tapes runs on the byte kernels
    // (only when both byte tapes have the same offset width: whether a UTF-8 call is accepted must not depend on what the
    // tapes contain -- a u32 / u64 mix falls back to the decoded tapes, whose offsets are always u64)
    bool utf8 = prepared ? (spec.pa->utf8 && !(spec.pa->ascii && spec.pb->ascii && spec.pa->off64 == spec.pb->off64)) : spec.utf8;
    size_t ow = prepared ? (utf8 ? 8 : (spec.pa->off64 ? 8 : 4)) : (spec.a.off64 ? 8 : 4), elem = spec.out64 ? 8 : 4;
    // residency of raw tapes (prepared ones are resident) and of the output; the tapes' byte totals where the call needs them
    bool dev_a_data = true, dev_a_off = true, dev_b_data = true, dev_b_off = true, same_tape = false, dev_out = false;
    bool need_sizes = false, believed_sizes = false;
    uint64_t a_bytes = 0, b_bytes = 0;
    // the tapes and the output as the kernels see them
    TapeRef ta{}, tb{};
    uint32_t sym_bytes = 1, off64 = 0;
    char *out_dev = nullptr;
    size_t dev_out_stride = 0, dev_row_stride = 0, out_bytes = 0;
    Lengths lengths;
    RouteChoice rc;
    uint32_t *invalid_dev = nullptr, *invalid_host = nullptr;   // UTF-8 staging flags: device words, their pinned copy
    bool staged_by_string = false;
    PrepassArgs pre{};
    KernelArgs k{};
    bool redo = false;   // the attempt is to be followed by another one, of `next`
    CallSpec next{};
    swh_status_t redo_with(const CallSpec &spec_of_next) { redo = true; next = spec_of_next; return swh_success_k; }

    // The attempt (its arguments passed check_call).
    swh_status_t attempt() {
        if (pairs == 0) return swh_success_k;
        if (prepared && !utf8 && spec.pa->off64 != spec.pb->off64)
            return fail(error, swh_invalid_argument_k, "prepared byte tapes must share one offset width");
        if (utf8 && engine->scoring.matrix)
            return fail(error, swh_not_implemented_k, "substitution-matrix scoring over UTF-8 code points (the matrix is indexed by bytes)");
        try {
            SWH_HIP_CHECK(hipSetDevice(scope->device));
            if (!prepared) {
                dev_a_data = is_device_pointer(spec.a.data); dev_a_off = is_device_pointer(spec.a.offsets);
                dev_b_data = is_device_pointer(spec.b.data); dev_b_off = is_device_pointer(spec.b.offsets);
                same_tape = spec.b.data == spec.a.data && spec.b.offsets == spec.a.offsets && spec.b.count == spec.a.count;
            }
            dev_out = is_device_pointer(spec.out);
            swh_status_t status = swh_success_k;
            if (ascii_shortcut(status)) return status;
            read_totals();
            place_buffers();
            lengths = call_lengths(scope, engine, spec, utf8);
            rc = pick_route(scope, engine, spec, utf8, dev_out, lengths);
            carve_scratch();
            if (spec.cross && spec.b.count >= 0xFFFFFFFFull) return fail(error, swh_unsupported_length_k, "more than 2^32 candidates");
            set_up_kernels();
            invalid_host = (uint32_t *)(scope->plan_host + 1);
            *invalid_host = 0;
            return rc.route == kRoutePlanned ? run_planned() : run_plan_free();
        } catch (const HipFailure &f) {
            return fail_hip(error, f);
        } catch (const std::bad_alloc &) {
            return fail(error, swh_bad_alloc_k, "host allocation failed");
        }
    }

    // Raw UTF-8 tapes that were pure ASCII the last time this scope staged them: code points of ASCII text are its bytes, so the call runs on
    // the byte kernels -- no staging, the word-sized and cross-product kernels instead of the code-point ones -- behind a kernel that checks
    // every byte of both tapes. True when that settled the call (`status`). False when it was not tried, or when a byte above 0x7F turned
    // up after all: the call then goes on the long way in the same attempt, after the byte kernels' stamps.
    // (Synchronous scopes only: an asynchronous call cannot be redone behind the caller's back.)
    bool ascii_shortcut(swh_status_t &status) {
        if (!(believe_sizes() && utf8 && !prepared && !scope->async && !spec.force_planned && dev_a_data && dev_a_off && dev_b_data &&
              dev_b_off && same_as_believed(spec.a, scope->size_belief[0]) && scope->size_belief[0].ascii &&
              (same_tape || (same_as_believed(spec.b, scope->size_belief[1]) && scope->size_belief[1].ascii))))
            return false;
        const Scope::SizeBelief &ba = scope->size_belief[0], &bb = same_tape ? scope->size_belief[0] : scope->size_belief[1];
        if (!allocation_covers(spec.a.data, ba.bytes) || !allocation_covers(spec.b.data, bb.bytes)) {
            (void)hipGetLastError();
            return false;
        }
        uint32_t *seen_host = (uint32_t *)((char *)scope->summary_host + 128), *seen_dev = (uint32_t *)((char *)scope->summary_dev + 128);
        *seen_host = 0;
        const uint64_t most = std::max<uint64_t>(ba.bytes, bb.bytes);
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((most + 4095) / 4096 + 1, (uint64_t)scope->compute_units * 8);
        hipLaunchKernelGGL(k_ascii_check, dim3(blocks), dim3(256), 0, stream, (const uint8_t *)spec.a.data, spec.a.offsets, (uint64_t)spec.a.count,
                           (const uint8_t *)spec.b.data, same_tape ? nullptr : spec.b.offsets, (uint64_t)spec.b.count, (uint32_t)spec.a.off64, seen_dev);
        SWH_HIP_CHECK(hipGetLastError());
        CallSpec as_bytes = spec;
        as_bytes.utf8 = false;
        status = run_call_on(scope, engine, as_bytes, error);
        // (the check ran in front of the byte kernels on the same stream: it is complete when their results are)
        if (status != swh_success_k || __atomic_load_n(seen_host, __ATOMIC_ACQUIRE) == 0) return true;
        scope->size_belief[0].ascii = scope->size_belief[1].ascii = false;
        scope->summary_pending = false;
        scope->stamps_pending = false;
        return false;
    }

    // The tapes' byte totals, where the call needs them before its first launch (scratch, grids): host tapes and raw UTF-8 tapes. A UTF-8
    // call on raw device tapes would pay two synchronous 4-byte copies for them, ~25 us of a 0.7 ms call: the same tapes as last time
    // (pointers, count) are believed to hold the same totals if the allocations still cover them; k_utf8_finish compares with
    // offsets[count] and the call is redone if not.
    void read_totals() {
        need_sizes = !prepared && (!dev_a_data || !dev_b_data || utf8);
        if (!need_sizes) return;
        const bool may_believe = believe_sizes() && utf8 && !spec.force_planned;
        auto total_of = [&](const HostTape &t, bool dev_data, bool dev_off, Scope::SizeBelief &slot) -> uint64_t {
            if (may_believe && dev_data && dev_off && same_as_believed(t, slot)) {
                if (allocation_covers(t.data, slot.bytes) && allocation_covers(t.offsets, (t.count + 1) * (t.off64 ? 8 : 4))) {
                    believed_sizes = true;
                    return slot.bytes;
                }
                (void)hipGetLastError();
            }
            const uint64_t bytes = read_offset(t.offsets, t.off64, t.count, dev_off, stream);
            remember_total(slot, t, bytes, dev_data && dev_off);
            return bytes;
        };
        // (two device tapes the scope has no belief about: both totals in ONE round trip -- two copies, one wait -- instead of two)
        const bool both_fresh = !same_tape && dev_a_off && dev_b_off && dev_a_data && dev_b_data &&
                                !(may_believe && (same_as_believed(spec.a, scope->size_belief[0]) || same_as_believed(spec.b, scope->size_belief[1])));
        if (both_fresh) {
            uint64_t *words = (uint64_t *)(scope->plan_host + 1) + 3;   // (pinned: bytes 24 .. 39 behind the plan; the UTF-8 flag words land in its first 20)
            words[0] = words[1] = 0;
            const size_t wa = spec.a.off64 ? 8 : 4, wb = spec.b.off64 ? 8 : 4;
            SWH_HIP_CHECK(hipMemcpyAsync(&words[0], (const char *)spec.a.offsets + spec.a.count * wa, wa, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipMemcpyAsync(&words[1], (const char *)spec.b.offsets + spec.b.count * wb, wb, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            a_bytes = words[0]; b_bytes = words[1];
            remember_total(scope->size_belief[0], spec.a, a_bytes, true);
            remember_total(scope->size_belief[1], spec.b, b_bytes, true);
        } else {
            a_bytes = total_of(spec.a, dev_a_data, dev_a_off, scope->size_belief[0]);
            b_bytes = same_tape ? a_bytes : total_of(spec.b, dev_b_data, dev_b_off, scope->size_belief[1]);
        }
    }

    // Where the kernels find the tapes and put the results: views of prepared tapes, device buffers in place, host buffers copied into the
    // scope's staging area. Device-resident outputs are written in place with the caller's strides; host outputs are produced compactly
    // in the staging area and scattered into the caller's strides by a 2-D copy (copy_results_back).
    void place_buffers() {
        dev_out_stride = dev_out ? spec.out_stride : elem;
        dev_row_stride = dev_out ? spec.row_stride : spec.b.count * elem;
        out_bytes = spec.cross ? (spec.a.count ? (spec.a.count - 1) * dev_row_stride + spec.b.count * elem : 0)
                           : (size_t)(pairs - 1) * dev_out_stride + elem;
        size_t stage_need = 0;
        if (!dev_a_data) stage_need += pad(a_bytes + 8);
        if (!dev_a_off) stage_need += pad((spec.a.count + 1) * ow + 8);
        if (!same_tape) {
            if (!dev_b_data) stage_need += pad(b_bytes + 8);
            if (!dev_b_off) stage_need += pad((spec.b.count + 1) * ow + 8);
        }
        if (!dev_out) stage_need += pad(out_bytes);
        ensure(scope->stage, scope->stage_bytes, stage_need);
        Carver st{scope->stage, 0, scope->stage_bytes};
        auto stage_in = [&](const void *src, size_t bytes, bool dev) -> const void * {
            if (dev) return src;
            char *dst = st.take<char>(bytes + 8);
            if (bytes) SWH_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
            return dst;
        };
        off64 = (uint32_t)spec.a.off64;
        if (prepared) {
            ta = prepared_view(spec.pa, utf8, spec.a_first, spec.a.count);
            tb = prepared_view(spec.pb, utf8, spec.b_first, spec.b.count);
            sym_bytes = utf8 ? 4 : 1;
            off64 = utf8 ? 1 : spec.pa->off64;
        } else {
            ta.data = stage_in(spec.a.data, a_bytes, dev_a_data);
            ta.offsets = stage_in(spec.a.offsets, (spec.a.count + 1) * ow, dev_a_off);
            ta.count = spec.a.count;
            if (same_tape) tb = ta;
            else {
                tb.data = stage_in(spec.b.data, b_bytes, dev_b_data);
                tb.offsets = stage_in(spec.b.offsets, (spec.b.count + 1) * ow, dev_b_off);
                tb.count = spec.b.count;
            }
        }
        out_dev = dev_out ? (char *)spec.out : st.take<char>(out_bytes);
    }

    // The call's scratch: the planned path's permutation and keys, then what the UTF-8 staging of raw tapes carves (stage_utf8).
    void carve_scratch() {
        const bool planned = rc.route == kRoutePlanned, staged = utf8 && !prepared;
        Carver probe{nullptr, 0, 0};
        if (planned) { probe.take<uint32_t>(pairs); probe.take<uint16_t>(pairs); }
        if (staged) {
            probe.take<uint32_t>(a_bytes + 4); probe.take<uint64_t>(spec.a.count + 1);
            probe.take<uint32_t>(utf8_scratch_words(a_bytes));
            probe.take<uint32_t>(b_bytes + 4); probe.take<uint64_t>(spec.b.count + 1);
            probe.take<uint32_t>(utf8_scratch_words(b_bytes));
            probe.take<uint32_t>(kUtf8FlagWords);
            probe.take<uint64_t>(2 * spec.a.count + 2); probe.take<uint64_t>(2 * spec.b.count + 2);   // (first, end) pairs of the string-by-string staging
        }
        ensure(scope->scratch, scope->scratch_bytes, probe.used);
        Carver sc{scope->scratch, 0, scope->scratch_bytes};
        if (planned) {
            pre.perm = sc.take<uint32_t>(pairs);
            k.perm = pre.perm;
            pre.keys = sc.take<uint16_t>(pairs);
        }
        if (staged) stage_utf8(sc);
    }

    // Raw UTF-8 tapes are decoded into code-point tapes in scratch before the DP launches.
    void stage_utf8(Carver &sc) {
        uint32_t decode_slot = 0;
        auto args_for = [&](const TapeRef &in, uint64_t bytes) {
            Utf8Args u{};
            u.slot = decode_slot++;
            u.in = in; u.off64 = off64; u.total_bytes = bytes;
            u.symbols = sc.take<uint32_t>(bytes + 4);
            u.offsets = sc.take<uint64_t>(in.count + 1);
            u.counts = sc.take<uint32_t>(utf8_scratch_words(bytes));
            u.invalid = invalid_dev;
            return u;
        };
        auto decoded = [](const Utf8Args &u) { return TapeRef{u.symbols, u.offsets, u.in.count}; };
        auto decode = [&](const TapeRef &in, uint64_t bytes, uint64_t first_word, bool opened) {
            const Utf8Args u = args_for(in, bytes);
            if (utf8_one_pass()) launch_utf8_decode_pair(scope, u, nullptr, first_word, opened);
            else launch_utf8_decode(scope, u);
            return decoded(u);
        };
        TapeRef da, db;
        invalid_dev = sc.take<uint32_t>(kUtf8FlagWords);   // one flag + two balance words + the tile tickets, shared by both decodes
        SWH_HIP_CHECK(hipMemsetAsync(invalid_dev, 0, kUtf8FlagWords * sizeof(uint32_t), stream));
        // Lines and longer strings are staged string by string (prepass.hip: k_utf8_strings -- one launch, no look-back; the code-point
        // tapes it leaves have gaps, TapeRef::gap): the routes whose kernels take their extents through pair_extent.
        const uint64_t all_strings = (uint64_t)spec.a.count + (same_tape ? 0 : spec.b.count), all_bytes = a_bytes + (same_tape ? 0 : b_bytes);
        if (scope->utf8_strings_rest) --scope->utf8_strings_rest;
        // (a too-long string sends the call back to the flat staging: the plan-free route can only do that where the host looks at the outcome)
        const Route route = rc.route;
        staged_by_string = (route == kRoutePlanned || (route == kRouteTiled && (!scope->async || !dev_out))) && utf8_strings_mode() != 2 && !spec.flat_staging &&
                             (utf8_strings_mode() == 1 || (scope->utf8_strings_rest == 0 && all_bytes >= (uint64_t)kUtf8StringsMeanBytes * all_strings));
        if (staged_by_string) {
            auto job_of = [&](const TapeRef &in, uint64_t bytes) {
                Utf8StringsJob j{};
                j.data = (const uint8_t *)in.data; j.offsets = in.offsets; j.count = in.count; j.total = bytes;
                j.symbols = sc.take<uint32_t>(bytes + 4);
                j.extents = sc.take<uint64_t>(2 * in.count + 2);
                return j;
            };
            const Utf8StringsJob sa = job_of(ta, a_bytes);
            da = TapeRef{sa.symbols, sa.extents, ta.count, 1};
            if (same_tape) {
                launch_utf8_strings(scope, sa, nullptr, off64, invalid_dev);
                db = da;
            } else {
                const Utf8StringsJob sb = job_of(tb, b_bytes);
                launch_utf8_strings(scope, sa, &sb, off64, invalid_dev);
                db = TapeRef{sb.symbols, sb.extents, tb.count, 1};
            }
        } else if (same_tape) {
            da = db = decode(ta, a_bytes, 0, false);
        } else if (utf8_one_pass() && a_bytes + b_bytes <= utf8_merged_bytes()) {
            // both tapes in the same two launches (tile decode, then string offsets + balance): what a small call costs is
            // its launches (10 K word pairs: 135 -> 107 us per call). Since the tile kernel draws from one ticket PER TAPE
            // (round 4) this is the path for every size (tools/mid_utf8.py, us per call, one launch pair : a launch pair and
            // a stream per tape -- 4 MB of tapes 186 : 205, 16 MB 216 : 240, 31 MB 256 : 283, 63 MB 330 : 352, 200 MB
            // 684 : 685); with one ticket for both tapes 2 x 100 MB took 0.33 ms in one launch against 0.27 in two.
            // STRINGWARS_AMD_UTF8_MERGED_MB=n sends tapes beyond n MB to the two-stream path below.
            const Utf8Args ua = args_for(ta, a_bytes), ub = args_for(tb, b_bytes);
            launch_utf8_decode_pair(scope, ua, &ub, 0, false);
            da = decoded(ua);
            db = decoded(ub);
        } else {
            // The two tapes decode side by side: the staging kernels are barrier- and latency-bound (half the issue
            // slots idle), so the second tape's run on the side stream, forked after the inputs are in place.
            struct StreamSwap {   // launch_utf8_decode and its event stamps follow scope->stream
                Scope *s; hipStream_t keep;
                StreamSwap(Scope *sc_, hipStream_t to) : s(sc_), keep(sc_->stream) { s->stream = to; }
                ~StreamSwap() { s->stream = keep; }
            };
            const uint64_t a_tiles = (a_bytes + kUtf8Tile - 1) / kUtf8Tile, b_tiles = (b_bytes + kUtf8Tile - 1) / kUtf8Tile;
            if (utf8_one_pass()) utf8_status_open(scope, a_tiles + b_tiles);   // before the fork: it may clear the words
            SWH_HIP_CHECK(hipEventRecord(scope->fork_ev, stream));
            SWH_HIP_CHECK(hipStreamWaitEvent(scope->side_stream, scope->fork_ev, 0));
            da = decode(ta, a_bytes, 0, true);
            {
                StreamSwap swap(scope, scope->side_stream);
                db = decode(tb, b_bytes, a_tiles, true);
            }
            SWH_HIP_CHECK(hipEventRecord(scope->join_ev, scope->side_stream));
            SWH_HIP_CHECK(hipStreamWaitEvent(stream, scope->join_ev, 0));
        }
        ta = da; tb = db;
        sym_bytes = 4; off64 = 1;
    }

    // The arguments of the planning pre-pass and of the DP kernels.
    void set_up_kernels() {
        Job job{};
        job.a = ta; job.b = tb; job.pairs = pairs; job.b_count = spec.b.count; job.cross = spec.cross ? 1 : 0;
        job.bound = engine->kind == 0 ? spec.bound : SWH_UNBOUNDED;
        job.out = out_dev; job.out_stride = dev_out_stride; job.row_stride = dev_row_stride;
        job.out_elem64 = spec.out64 ? 1 : 0;
        job.negate = engine->kind == 0 ? 1 : 0;
        if (spec.cross) cross_divider((uint32_t)spec.b.count, job.div_magic, job.div_shift);

        pre.job = job;
        pre.mode = bitpar_ok ? kPlanBitParallel : kPlanWavefront;
        pre.off64 = off64; pre.sym_bytes = sym_bytes;
        pre.symmetric = engine->kind == 0 ? 1u : (engine->unit_costs ? 1u : 0u);  // nw: set at init when symmetric
        pre.gap_open = engine->scoring.open; pre.gap_extend = engine->scoring.extend;
        pre.unit_costs = engine->kind == 0 && engine->unit_costs ? 1 : 0;
        pre.local = engine->kind == 2 ? 1 : 0;
        pre.direct_short = bitpar_ok && sym_bytes == 1 && engine->algorithm == swh_algorithm_auto_k && scope->hint_short ? 1 : 0;
        pre.skip_upto = spec.skip_upto;
        pre.banded = pre.unit_costs && spec.bound <= band_max_bound() && engine->algorithm == swh_algorithm_auto_k ? 1 : 0;
        pre.hist = scope->plan_hist; pre.cursor = scope->plan_cursor;
        pre.partials = scope->plan_partials; pre.leftover = scope->plan_leftover; pre.plan = scope->plan_dev;

        k.job = job; k.plan = scope->plan_dev; k.scoring = engine->scoring;
        k.off64 = off64; k.sym_bytes = sym_bytes; k.symmetric = pre.symmetric;
        k.affine = engine->scoring.open != engine->scoring.extend ? 1 : 0;
        k.local = engine->kind == 2 ? 1 : 0;
    }

    void copy_results_back() const {
        if (dev_out) return;
        if (spec.cross) {
            SWH_HIP_CHECK(hipMemcpy2DAsync(spec.out, spec.row_stride, out_dev, dev_row_stride, spec.b.count * elem,
                                           spec.a.count, hipMemcpyDeviceToHost, stream));
        } else if (spec.out_stride == elem) {
            SWH_HIP_CHECK(hipMemcpyAsync(spec.out, out_dev, out_bytes, hipMemcpyDeviceToHost, stream));
        } else {
            SWH_HIP_CHECK(hipMemcpy2DAsync(spec.out, spec.out_stride, out_dev, elem, elem, pairs, hipMemcpyDeviceToHost, stream));
        }
    }
    // what the staging saw of the tapes' bytes (one-pass kernel only): the next call on the same tapes may believe it
    void learn_ascii() const {
        if (!invalid_dev || !utf8_one_pass()) return;
        if (same_as_believed(spec.a, scope->size_belief[0])) scope->size_belief[0].ascii = invalid_host[kUtf8AsciiWord] == 0;
        if (!same_tape && same_as_believed(spec.b, scope->size_belief[1])) scope->size_belief[1].ascii = invalid_host[kUtf8AsciiWord + 1] == 0;
    }
    // The UTF-8 staging raised its flag: the call is redone where what it believed did not hold, else the input is invalid.
    swh_status_t utf8_flagged() {
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        const uint32_t marker = *invalid_host;
        if (marker == kUtf8SizesChanged && believed_sizes) {
            // the tapes changed behind the belief: read their totals afresh and do the call again
            scope->size_belief[0].valid = scope->size_belief[1].valid = false;
            return redo_with(spec);
        }
        if (marker == kUtf8StringTooLong && staged_by_string) {
            // a string too long for a wave of its own (k_utf8_strings): this call and the scope's next few stage the flat way
            scope->utf8_strings_rest = 16;
            CallSpec flat = spec;
            flat.flat_staging = true;
            return redo_with(flat);
        }
        return fail(error, swh_invalid_utf8_k, "invalid UTF-8 in an input tape (marker %u: the string's index when staged string by string, else a 4-byte word inside the 1 KiB tile that failed)", marker - 1);
    }

    // No pre-pass: one DP launch; its summary (work units, longest strings, "a pair did not fit") arrives in host-mapped memory with the
    // kernel's completion. A synchronous call whose belief about the lengths did not hold is redone on the planned path.
    swh_status_t run_plan_free() {
        const Route route = rc.route;
        const uint32_t longest = rc.longest;
        // (an asynchronous call reports into slot 1, whose `sticky` word outlives the summary: see CallSummary)
        scope->summary_slot = (scope->async && dev_out) ? 1u : 0u;
        const bool early = !scope->async && dev_out && !scope->profiling && !invalid_dev && early_return_on() && is_plain_device_memory(spec.out, scope->device);
        if (early) scope->summary_host[0].landed = 0;
        if (route == kRouteDirectShort) launch_direct_short_alone(scope, pre);
        else if (route == kRouteShortTiled) {
            // mean string length, for the chunk size: exact for prepared tapes (their totals), else what the last call saw
            const uint32_t mean_x16 = prepared ? (uint32_t)std::min<uint64_t>(lengths.prepared_mean_x16, 0xFFFFFFu) : scope->hint_mean_x16;
            launch_short_tiled(scope, pre.job, off64, mean_x16);
        }
        else if (route == kRouteCrossShort) launch_cross_short(scope, pre.job, off64, sym_bytes);
        else if (route == kRouteAlignShort) launch_align_short(scope, k, longest, rc.align_wide);
        else if (route == kRouteAlignLong) {
            const uint32_t per_item = align_long_queries(scope, spec.a.count, spec.b.count);
            const uint64_t items = ((uint64_t)(spec.b.count + 63) / 64) * ((uint64_t)(spec.a.count + per_item - 1) / per_item);
            const uint64_t ints = (uint64_t)align_long_waves(scope, items, longest, k.affine != 0) * (longest + 8) * 64 * (k.affine ? 2 : 1);
            ensure(scope->boundary, scope->boundary_bytes, ints * sizeof(int32_t));
            k.boundary = (int32_t *)scope->boundary;
            launch_align_long(scope, k, longest);
        }
        else launch_bitparallel_tiled(scope, k, pairs, longest);
        if (invalid_dev) SWH_HIP_CHECK(hipMemcpyAsync(invalid_host, invalid_dev, 4 * (kUtf8AsciiWord + 2), hipMemcpyDeviceToHost, stream));
        copy_results_back();
        scope->summary_sym_bytes = need_sizes ? 0 : sym_bytes;
        scope->summary_pairs = pairs; scope->summary_ow = ow; scope->summary_elem = elem;
        scope->summary_strings = spec.cross ? (uint64_t)spec.a.count + spec.b.count : 2 * (uint64_t)pairs;
        scope->summary_extra_bytes = need_sizes ? a_bytes + b_bytes : 0;
        scope->summary_pending = true;
        scope->stamps_pending = scope->profiling;
        if (scope->async && dev_out) return swh_success_k;
        if (early) wait_for_summary(scope, stream);
        else SWH_HIP_CHECK(hipStreamSynchronize(stream));
        if (*invalid_host) return utf8_flagged();
        learn_ascii();
        if (scope->summary_host[0].max_la >= kStringLimit || scope->summary_host[0].max_lb >= kStringLimit) {
            // A string the windows cannot index (common.hpp: kStringLimit). The kernels of these routes leave its pair alone, or -- where
            // they finish the pairs that lengths alone decide (k_direct_short) -- store a value that means nothing: the call is refused
            // here as the planned path refuses it, and the scope believes nothing about this batch.
            scope->summary_pending = false;
            scope->stamps_pending = false;
            scope->hint_lengths = false;
            return fail(error, swh_unsupported_length_k, "a string of 2^30 symbols or more (the longest: %u x %u symbols)",
                        scope->summary_host[0].max_la, scope->summary_host[0].max_lb);
        }
        if (scope->summary_host[0].violation) {
            // the belief about the lengths was wrong (it came from an earlier batch): redo on the planned path
            scope->hint_lengths = false;
            // the compacting kernels stay off this scope only when the ALPHABET was the reason (violation bit 1); a string longer
            // than the believed lengths just drops the belief, and the next batch of the same shape is routed afresh
            const bool compact_route = (route == kRouteAlignShort && rc.align_wide) || route == kRouteAlignLong;
            const bool compact_failed = compact_route && (scope->summary_host[0].violation & 2u) != 0;
            if (compact_failed) {
                scope->align_wide_off.engine = engine->uid;
                scope->align_wide_off.a = spec.pa ? (const void *)spec.pa : (const void *)spec.a.data;
                scope->align_wide_off.b = spec.pb ? (const void *)spec.pb : (const void *)spec.b.data;
            }
            CallSpec again = spec;
            // (prepared tapes know their lengths: when only the small-alphabet kernels' condition failed, the redo may still take
            // the lane-per-pair kernel -- `align_wide_off` keeps it off the compacting ones)
            again.force_planned = !(compact_failed && prepared);
            // the lane-per-pair kernel has scored every pair whose two strings fit its register row: the redo plans the others
            if (route == kRouteAlignShort && !rc.align_wide) again.skip_upto = longest <= 16 ? 16u : (longest <= 32 ? 32u : 64u);
            return redo_with(again);
        }
        harvest_timing(scope, true);
        return swh_success_k;
    }

    // Doubling. A unit-cost call whose bound lies beyond one band word (or that has none) first runs the ONE-WORD band at k1 = 63 over
    // the pairs long enough for it: whatever comes back <= 63 is the distance, under any larger bound, and only the pairs that
    // came back 64 are planned again with the call's own bound (two-word band, bit-parallel blocks). The reference's CPU row does
    // the same inside every call -- rapidfuzz doubles a score hint of 31 until the result fits under it -- and text that is compared
    // for similarity mostly is similar: config C3's lines, unbounded, 26 -> ~50 TCUPS. The first stage costs band_cost(63) per
    // column where the second costs `later`; the share of pairs it has to settle for that to pay (plus a quarter: a second plan, a
    // second tail) is held against what the scope's previous doubling call saw, and a scope that saw less sits eight calls out.
    Doubling decide_doubling() const {
        static const bool doubling_on = [] { const char *e = test_hook("STRINGWARS_AMD_DOUBLING"); return !e || atoi(e) != 0; }();
        static const uint64_t doubling_min = [] { const char *e = test_hook("STRINGWARS_AMD_DOUBLING_MIN"); return e ? (uint64_t)atoll(e) : (uint64_t)200000; }();   // tuning knob: pairs x blocks
        Doubling d;
        if (!(doubling_on && bitpar_ok && pre.unit_costs && engine->algorithm == swh_algorithm_auto_k && spec.bound > kDoublingBound && lengths.known))
            return d;
        const uint32_t blocks = (std::min(lengths.la_max, lengths.lb_max) + 31) >> 5;
        const uint32_t unbounded_cost = (sym_bytes == 4 ? 40u : 28u) * blocks;
        const uint32_t later = spec.bound <= band_max_bound() ? std::min(band_cost(spec.bound), unbounded_cost) : unbounded_cost;
        d.need = 1.25 * band_cost(kDoublingBound) / std::max(later, 1u);
        if (scope->doubling_rest) --scope->doubling_rest;
        else d.on = d.need <= 0.95 && (uint64_t)pairs * blocks >= doubling_min;   // (a second plan and a second tail: not for small batches)
        return d;
    }

    // The planned path: classify + counting sort on the device, then the DP kernels the plan's classes call for.
    swh_status_t run_planned() {
        const Doubling doubling = decide_doubling();
        if (doubling.on) {
            PrepassArgs first = pre;
            first.job.bound = kDoublingBound; first.banded = 1; first.stage1 = 1; first.direct_short = 0; first.skip_upto = 0;
            launch_prepass(scope, first);
            KernelArgs kf = k;
            kf.job.bound = kDoublingBound;
            launch_banded(scope, kf, pairs);
            pre.redo_filter = 1; pre.redo_done_upto = kDoublingBound;
            // What is left after a first stage that settles nearly everything is a few thousand pairs: too few to fill the device with
            // the two-word band's items (one wave walks a pair's every column: C3's lines at k = 100, 2 % left over, 0.19 ms), while a
            // bit-parallel item spreads ONE pair over the lanes of its blocks (0.07 ms). Where the scope's previous doubling call left
            // less than a tenth, the second stage plans without the band (the results are clamped to the bound either way).
            if (scope->doubling_settled >= 0.9f) pre.banded = 0;
        }
        launch_prepass(scope, pre);
        // The bit-parallel kernel reads its work list from the device plan, so it is enqueued right away;
        // the host copy of the plan (needed only to pick wavefront kernels) travels on a side stream and
        // overlaps it.
        SWH_HIP_CHECK(hipEventRecord(scope->plan_ready, stream));
        if (pre.banded) launch_banded(scope, k, pairs);
        // Bounded calls: the banded kernel keeps the device busy while the plan travels, so the bit-parallel launch waits until
        // the host knows whether it has any pairs at all (C3: none -- an empty launch and its gap were 8 us of a 0.4 ms call).
        const bool bitpar_deferred = bitpar_ok && pre.banded;
        if (bitpar_ok && !bitpar_deferred) launch_bitparallel(scope, k, pairs);
        Plan &plan = *scope->plan_host;
        SWH_HIP_CHECK(hipStreamWaitEvent(scope->side_stream, scope->plan_ready, 0));
        SWH_HIP_CHECK(hipMemcpyAsync(&plan, scope->plan_dev, sizeof(Plan), hipMemcpyDeviceToHost, scope->side_stream));
        if (invalid_dev)
            SWH_HIP_CHECK(hipMemcpyAsync(invalid_host, invalid_dev, 4 * (kUtf8AsciiWord + 2), hipMemcpyDeviceToHost, scope->side_stream));
        SWH_HIP_CHECK(hipStreamSynchronize(scope->side_stream));
        if (plan.fused_failed) {
            // the one-launch planner could not gather its grid (a device shared with long-running foreign kernels): the DP
            // kernels found an empty plan; plan again with the three passes, now and from here on
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            scope->fused_disabled = true;
            return redo_with(spec);
        }
        if (plan.max_la >= kStringLimit || plan.max_lb >= kStringLimit) {
            // (the planner filed the pairs of such strings as done: nothing walks them; the other pairs' results may have been written)
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            return fail(error, swh_unsupported_length_k, "a string of 2^30 symbols or more (the longest: %u x %u symbols)", plan.max_la, plan.max_lb);
        }
        // enqueue k_direct_short next time only if short pairs are a real share of the batch (it sweeps all offsets)
        scope->hint_short = (uint64_t)plan.short_pairs * 4 >= pairs;
        scope->hint_lengths = true;
        scope->hint_max_la = plan.max_la; scope->hint_max_lb = plan.max_lb;
        {
            const uint64_t strings = 2 * (uint64_t)pairs;   // (the planner sums la + lb over PAIRS, also for a cross-product)
            scope->hint_mean_string_x16 = strings ? (uint32_t)std::min<uint64_t>(plan.symbols * 16 / strings, 0xFFFFFFu) : 0u;
        }
        if (*invalid_host) return utf8_flagged();
        learn_ascii();
        if (doubling.on) {
            // what the first stage left over: the pairs the second plan filed under a kernel class
            const uint64_t left = plan.class_start[kMaxClasses] - plan.class_count[kClassTrivial];
            const double settled = 1.0 - (double)left / (double)pairs;
            scope->doubling_settled = (float)settled;
            if (settled < doubling.need) scope->doubling_rest = 8;
        }

        if (bitpar_deferred) {
            bool any_bp = false;
            for (int cls = kClassBp0; cls < kClassBp0 + 64; ++cls) any_bp |= plan.class_count[cls] != 0;
            if (any_bp) launch_bitparallel(scope, k, pairs);
        }
        // patterns of more than 64 blocks: multi-pass bit-parallel kernel, carries between passes in scratch
        if (bitpar_ok && plan.class_count[kClassBpLong]) {
            const uint64_t stride = bp_long_carry_words(plan.max_la > plan.max_lb ? plan.max_la : plan.max_lb);
            // one carry area per wave the launch can have: ceil(count / waves-per-block) blocks of 4 (bytes) or 11 (code points) waves
            const uint64_t waves = plan.class_count[kClassBpLong] + 16 < kBpLongMaxWaves ? plan.class_count[kClassBpLong] + 16 : kBpLongMaxWaves;
            ensure(scope->boundary, scope->boundary_bytes, waves * stride * sizeof(uint32_t));
            KernelArgs kl = k;
            kl.boundary = (int32_t *)scope->boundary;
            kl.boundary_stride = stride;
            launch_bitparallel_long(scope, kl, plan);
        }

        // Global or local alignment on a class table (<= 32 symbol classes; 33 .. 128 on the wide table), pairs of more than 384 columns: the column-profile kernel
        // (nwprofile.hip) takes them -- perm is sorted by class, so they are one contiguous range -- and the wavefront
        // kernels below see a plan without them. STRINGWARS_AMD_NW=classic keeps everything on the wavefront kernels.
        static const bool nw_classic = [] { const char *e = test_hook("STRINGWARS_AMD_NW"); return e && strcmp(e, "classic") == 0; }();
        uint32_t profile_first = 0, profile_count = 0;
        Plan wf_plan = plan;
        if ((engine->kind == 1 || engine->kind == 2) && (engine->scoring.class_table || engine->scoring.wide_table) && sym_bytes == 1 && !nw_classic) {
            profile_first = plan.class_start[kClassWf64 + kNwProfileFirstWide];
            for (int cls = kClassWf64 + kNwProfileFirstWide; cls <= kClassWfMulti; ++cls) { profile_count += plan.class_count[cls]; wf_plan.class_count[cls] = 0; }
        }
        // wavefront classes (all of them when the plan is wavefront-only)
        bool any_wf = false, multi = false;
        for (int cls = kClassWf16; cls <= kClassWfMulti; ++cls) {
            if (!wf_plan.class_count[cls]) continue;
            any_wf = true;
            if (cls == kClassWfMulti || (k.affine && cls >= kClassWf64 + 8)) multi = true;  // (affine strips are capped: the widest classes take several passes)
            if (wavefront_strip_cap() && cls >= kClassWf64 && wide_w(cls - kClassWf64 < kNumWideW ? cls - kClassWf64 : kNumWideW - 1) > wavefront_strip_cap()) multi = true;
        }
        if (any_wf || profile_count) {
            // int32 scores with a -2^29 "minus infinity": keep every reachable score well inside it
            const uint64_t worst_step = std::max<uint64_t>({(uint64_t)std::abs(engine->scoring.open), (uint64_t)std::abs(engine->scoring.extend),
                                                            (uint64_t)std::abs(engine->scoring.match), (uint64_t)std::abs(engine->scoring.mismatch),
                                                            engine->scoring.matrix ? 128u : 0u});
            if (worst_step * ((uint64_t)plan.max_la + plan.max_lb + 2) >= 0x10000000ull) {
                SWH_HIP_CHECK(hipStreamSynchronize(stream));
                return fail(error, swh_unsupported_length_k, "scores of this batch could leave the 32-bit range of the wavefront kernels (costs x lengths too large)");
            }
            // one boundary column (H, E) per concurrently resident group: two areas for the wavefront class kernels, which
            // alternate between two streams and run side by side (launch_wavefront), one for the profile kernel's waves
            const uint64_t stride = (uint64_t)(plan.max_la > plan.max_lb ? plan.max_la : plan.max_lb) + 64 + 16;
            const uint64_t groups = multi ? (uint64_t)scope->compute_units * 8 * 4 : 0;  // max blocks * waves (G = 64)
            // (one area per wave the profile launch can have: launch_nwprofile never starts more workgroups than it has pairs)
            const uint64_t profile_waves = profile_count ? std::min<uint64_t>(nwprofile_waves(scope, engine->scoring.classes ? engine->scoring.classes : 32), profile_count) : 0;
            if (multi || profile_count) ensure(scope->boundary, scope->boundary_bytes, (2 * groups + profile_waves) * stride * 2 * sizeof(int32_t));
            if (profile_count) {
                KernelArgs kp = k;
                kp.boundary = (int32_t *)scope->boundary + 2 * groups * stride * 2;
                kp.boundary_stride = stride;
                if (kp.local && engine->scoring.step_span) {
                    // Scoring::step_span = largest |cost| - open - extend (alignment_init): a local score is at most the largest cost x the shorter string
                    const uint64_t largest_cost = (uint64_t)((int64_t)engine->scoring.step_span + engine->scoring.open + engine->scoring.extend);
                    kp.local_narrow = largest_cost * (uint64_t)std::min(plan.max_la, plan.max_lb) < 0xFFFFull ? 1u : 0u;
                }
                launch_nwprofile(scope, kp, profile_first, profile_count);
            }
            if (multi) {
                k.boundary = (int32_t *)scope->boundary;
                k.boundary_stride = stride;
                scope->wf_side_boundary = groups * stride * 2;
            }
            if (any_wf) launch_wavefront(scope, k, wf_plan);
        }

        copy_results_back();
        scope->last_timing.cells = plan.cells;
        scope->last_timing.bytes = (need_sizes ? a_bytes + b_bytes : plan.symbols * sym_bytes) + pairs * (2 * ow + elem);
        scope->stamps_pending = scope->profiling;
        if (!scope->async || !dev_out) {
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            harvest_timing(scope, true);
        }
        return swh_success_k;
    }
};

static swh_status_t run_call_on(Scope *scope, const Engine *engine, const CallSpec &first, const char **error) {
    const swh_status_t checked = check_call(scope, engine, first, error);
    if (checked != swh_success_k) return checked;
    CallSpec spec = first;
    for (;;) {
        harvest_timing(scope, false);   // an earlier asynchronous call on this scope / lane
        scope->stamps_used = 0;
        scope->last_timing = swh_timing_t{};
        Call call{scope, engine, spec, error};
        const swh_status_t status = call.attempt();
        if (!call.redo) return status;
        scope->summary_pending = false;
        scope->stamps_pending = false;
        spec = call.next;
    }
}

}  // namespace swh

using namespace swh;

// Alignment scratch (align.hip) of every scope that ran an alignment: stored delta vectors, op slots, scans. Kept here rather than in
// Scope so that common.hpp -- which every kernel family's profile stamp hashes -- stays as it is; freed with the scope.
struct AlignScratch { char *buf = nullptr; size_t bytes = 0; };
static std::mutex g_align_scratch_lock;
static std::unordered_map<const Scope *, AlignScratch> g_align_scratch;
static void free_align_scratch(const Scope *scope) {
    std::lock_guard<std::mutex> hold(g_align_scratch_lock);
    auto it = g_align_scratch.find(scope);
    if (it == g_align_scratch.end()) return;
    if (it->second.buf) (void)hipFree(it->second.buf);
    g_align_scratch.erase(it);
}

// =====================================================================================================
// extern "C"
// =====================================================================================================
extern "C" {

const char *swh_version(void) { return "0.1.0"; }
const char *swh_capabilities(void) { return "gfx950,hip,wavefront,bitparallel,tiled,banded,utf8,bounded,nw-linear,nw-affine,sw-linear,sw-affine,cross,prepared,topk,within,align,infix,osa,lcs,jaro,extract,multi-gpu-rccl"; }

static swh_status_t scope_init(int device, void *stream, bool borrow, swh_scope_t *out, const char **error) {
    if (!out) return fail(error, swh_invalid_argument_k, "null scope pointer");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        (void)hipGetLastError();
        return fail(error, swh_no_device_k, "no HIP device visible (this backend has no CPU path)");
    }
    if (device < 0 || device >= count) return fail(error, swh_no_device_k, "HIP device index out of range");
    try {
        SWH_HIP_CHECK(hipSetDevice(device));
        hipDeviceProp_t prop;
        SWH_HIP_CHECK(hipGetDeviceProperties(&prop, device));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(error, swh_no_device_k, "device is %s, this library carries gfx950 code only", prop.gcnArchName);
        Scope *scope = new Scope();
        scope->device = device;
        scope->compute_units = prop.multiProcessorCount;
        if (borrow) { scope->stream = (hipStream_t)stream; scope->owns_stream = false; }
        else { SWH_HIP_CHECK(hipStreamCreateWithFlags(&scope->stream, hipStreamNonBlocking)); scope->owns_stream = true; }
        SWH_HIP_CHECK(hipHostMalloc((void **)&scope->plan_host, sizeof(Plan) + 64, hipHostMallocDefault));
        {   // plan area: hist | cursor | partials | leftover + done counter | plan; zeroed once (the kernels re-zero what they use)
            Carver measure{nullptr, 0, 0};
            measure.take<uint32_t>(kKeys); measure.take<uint32_t>(kKeys); measure.take<PlanPartial>(2 * kMaxPartials);
            measure.take<uint32_t>(8); measure.take<Plan>(1);
            measure.take<uint32_t>(kKeys); measure.take<uint32_t>(kKeys); measure.take<uint32_t>(4);
            SWH_HIP_CHECK(hipMalloc((void **)&scope->plan_area, measure.used));
            SWH_HIP_CHECK(hipMemset(scope->plan_area, 0, measure.used));
            Carver pa{scope->plan_area, 0, measure.used};
            scope->plan_hist = pa.take<uint32_t>(kKeys);
            scope->plan_cursor = pa.take<uint32_t>(kKeys);
            scope->plan_partials = pa.take<PlanPartial>(2 * kMaxPartials);
            scope->plan_leftover = pa.take<uint32_t>(8);
            scope->done_counter = scope->plan_leftover + 4;
            scope->plan_dev = pa.take<Plan>(1);
            scope->plan_hist2[0] = pa.take<uint32_t>(kKeys);
            scope->plan_hist2[1] = pa.take<uint32_t>(kKeys);
            scope->plan_barrier = pa.take<uint32_t>(4);
        }
        // summary of plan-free calls: pinned, mapped, coherent -- the kernels write it, the host reads it after synchronising
        SWH_HIP_CHECK(hipHostMalloc((void **)&scope->summary_host, 256, hipHostMallocMapped | hipHostMallocCoherent));
        memset(scope->summary_host, 0, 256);
        SWH_HIP_CHECK(hipHostGetDevicePointer((void **)&scope->summary_dev, scope->summary_host, 0));
        SWH_HIP_CHECK(hipStreamCreateWithFlags(&scope->side_stream, hipStreamNonBlocking));
        SWH_HIP_CHECK(hipEventCreateWithFlags(&scope->plan_ready, hipEventDisableTiming));
        SWH_HIP_CHECK(hipEventCreateWithFlags(&scope->fork_ev, hipEventDisableTiming));
        SWH_HIP_CHECK(hipEventCreateWithFlags(&scope->join_ev, hipEventDisableTiming));
        *out = (swh_scope_t)scope;
        return swh_success_k;
    } catch (const HipFailure &f) {
        return fail_hip(error, f);
    }
}

swh_status_t swh_scope_init_gpu(int device, swh_scope_t *scope, const char **error) {
    return scope_init(device, nullptr, false, scope, error);
}
swh_status_t swh_scope_init_gpu_stream(int device, void *hip_stream, swh_scope_t *scope, const char **error) {
    return scope_init(device, hip_stream, true, scope, error);
}
swh_status_t swh_scope_init_cpu(size_t, swh_scope_t *scope, const char **error) {
    if (scope) *scope = nullptr;
    return fail(error, swh_not_implemented_k, "stringwars_amd has no CPU backend; use a GPU scope");
}
swh_status_t swh_scope_free(swh_scope_t handle) {
    Scope *scope = (Scope *)handle;
    if (!scope) return swh_success_k;
    for (Scope *&lane : scope->lanes)
        if (lane) { swh_scope_free((swh_scope_t)lane); lane = nullptr; }
    if (scope->multi) { free_multi_scope(scope->multi); scope->multi = nullptr; }
    (void)hipSetDevice(scope->device);
    (void)hipStreamSynchronize(scope->stream);
    if (scope->lane_done) (void)hipEventDestroy(scope->lane_done);
    if (scope->order_ev) (void)hipEventDestroy(scope->order_ev);
    for (auto &st : scope->stamps) { (void)hipEventDestroy(st.start); (void)hipEventDestroy(st.stop); }
    if (scope->scratch) (void)hipFree(scope->scratch);
    if (scope->utf8_status) (void)hipFree(scope->utf8_status);
    if (scope->stage) (void)hipFree(scope->stage);
    if (scope->boundary) (void)hipFree(scope->boundary);
    if (scope->topk_scratch) (void)hipFree(scope->topk_scratch);
    if (scope->within_out) (void)hipFree(scope->within_out);
    free_align_scratch(scope);
    if (scope->plan_host) (void)hipHostFree(scope->plan_host);
    if (scope->summary_host) (void)hipHostFree(scope->summary_host);
    if (scope->plan_area) (void)hipFree(scope->plan_area);
    if (scope->side_stream) (void)hipStreamDestroy(scope->side_stream);
    if (scope->fork_ev) (void)hipEventDestroy(scope->fork_ev);
    if (scope->join_ev) (void)hipEventDestroy(scope->join_ev);
    if (scope->plan_ready) (void)hipEventDestroy(scope->plan_ready);
    if (scope->owns_stream) (void)hipStreamDestroy(scope->stream);
    delete scope;
    return swh_success_k;
}
swh_status_t swh_scope_compute_units(swh_scope_t handle, size_t *cus) {
    if (!handle || !cus) return swh_invalid_argument_k;
    *cus = (size_t)((Scope *)handle)->compute_units;
    return swh_success_k;
}
swh_status_t swh_scope_set_async(swh_scope_t handle, int async) {
    if (!handle) return swh_invalid_argument_k;
    ((Scope *)handle)->async = async != 0;
    return swh_success_k;
}
swh_status_t swh_scope_synchronize(swh_scope_t handle, const char **error) {
    Scope *scope = (Scope *)handle;
    if (!scope) return fail(error, swh_invalid_argument_k, "null scope");
    bool violated = false;
    for (Scope *lane : scope->lanes)
        if (lane) {
            hipError_t lerr = hipStreamSynchronize(lane->stream);
            if (lerr != hipSuccess) return fail_hip(error, HipFailure{lerr, "hipStreamSynchronize (lane)"});
            harvest_timing(lane, true);
            violated |= lane->violation_seen; lane->violation_seen = false;
        }
    hipError_t err = hipStreamSynchronize(scope->stream);
    if (err != hipSuccess) return fail_hip(error, HipFailure{err, "hipStreamSynchronize"});
    harvest_timing(scope, true);
    violated |= scope->violation_seen; scope->violation_seen = false;
    // every asynchronous plan-free call since the last synchronisation, not only the one whose summary was still there to read
    for (Scope *each : {scope, scope->lanes[0], scope->lanes[1]})
        if (each && each->summary_host && each->summary_host[1].sticky) { violated = true; each->summary_host[1].sticky = 0; }
    if (scope->pipelined && scope->last_lane) scope->last_timing = scope->last_lane->last_timing;
    if (violated)
        return fail(error, swh_invalid_argument_k, "an asynchronous call met strings longer than its prepared tapes were measured with (was a tape's memory "
                                                   "changed after swh_tape_prepare_*?): those pairs were not scored");
    return swh_success_k;
}
swh_status_t swh_scope_set_pipelined(swh_scope_t handle, int enabled, const char **error) {
    Scope *scope = (Scope *)handle;
    if (!scope) return fail(error, swh_invalid_argument_k, "null scope");
    swh_status_t status = swh_scope_synchronize(handle, error);
    if (status != swh_success_k) return status;
    if (enabled) {
        if (!scope->order_ev && hipEventCreateWithFlags(&scope->order_ev, hipEventDisableTiming) != hipSuccess)
            return fail(error, swh_device_error_k, "hipEventCreate failed for the pipeline");
        for (Scope *&lane : scope->lanes) {
            if (lane) continue;
            swh_scope_t created = nullptr;
            status = swh_scope_init_gpu(scope->device, &created, error);   // own non-blocking stream + buffers
            if (status != swh_success_k) return status;
            lane = (Scope *)created;
            lane->async = true;
            lane->profiling = scope->profiling;
            if (hipEventCreateWithFlags(&lane->lane_done, hipEventDisableTiming) != hipSuccess)
                return fail(error, swh_device_error_k, "hipEventCreate failed for a pipeline lane");
        }
    }
    scope->pipelined = enabled != 0;
    scope->last_lane = nullptr;
    return swh_success_k;
}
swh_status_t swh_scope_join(swh_scope_t handle, const char **error) {
    Scope *scope = (Scope *)handle;
    if (!scope) return fail(error, swh_invalid_argument_k, "null scope");
    if (!scope->pipelined || !scope->last_lane) return swh_success_k;   // calls already ran on the scope's own stream
    hipError_t err = hipStreamWaitEvent(scope->stream, scope->last_lane->lane_done, 0);
    if (err != hipSuccess) return fail_hip(error, HipFailure{err, "hipStreamWaitEvent"});
    return swh_success_k;
}
swh_status_t swh_scope_forget(swh_scope_t handle) {
    if (!handle) return swh_invalid_argument_k;
    Scope *scope = (Scope *)handle;
    Scope *all[3] = {scope, scope->lanes[0], scope->lanes[1]};
    for (Scope *s : all) {
        if (!s) continue;
        s->hint_short = true;
        s->hint_lengths = false;
        s->hint_max_la = s->hint_max_lb = 0;
        s->hint_mean_x16 = s->hint_mean_string_x16 = 0;
        s->size_belief[0] = Scope::SizeBelief{};
        s->size_belief[1] = Scope::SizeBelief{};
        s->doubling_settled = -1.0f;
        s->doubling_rest = 0;
        s->utf8_strings_rest = 0;
        s->align_wide_off = Scope::AlignWideOff{};
        s->early_return_last_us = 0;
    }
    return swh_success_k;
}
swh_status_t swh_scope_describe(swh_scope_t handle, char *text, size_t capacity) {
    if (!handle || !text || !capacity) return swh_invalid_argument_k;
    const Scope *s = (const Scope *)handle;
    snprintf(text, capacity,
             "lengths_believed=%d longest_a=%u longest_b=%u mean_string_x16=%u short_pairs_expected=%d "
             "utf8_tape0=%s%s utf8_tape1=%s%s doubling_settled=%.3f doubling_rest=%u utf8_strings_rest=%u "
             "align_wide_off_engine=%llu fused_planner=%s",
             s->hint_lengths ? 1 : 0, s->hint_max_la, s->hint_max_lb, s->hint_mean_string_x16, s->hint_short ? 1 : 0,
             s->size_belief[0].valid ? "sized" : "unknown", s->size_belief[0].ascii ? "+ascii" : "",
             s->size_belief[1].valid ? "sized" : "unknown", s->size_belief[1].ascii ? "+ascii" : "",
             (double)s->doubling_settled, s->doubling_rest, s->utf8_strings_rest,
             (unsigned long long)s->align_wide_off.engine, s->fused_disabled ? "off" : "on");
    return swh_success_k;
}
swh_status_t swh_scope_set_profiling(swh_scope_t handle, int enabled) {
    if (!handle) return swh_invalid_argument_k;
    Scope *scope = (Scope *)handle;
    Scope *all[3] = {scope, scope->lanes[0], scope->lanes[1]};
    for (Scope *s : all) {
        if (!s) continue;
        if (enabled && !s->profiling) { s->totals = swh_timing_totals_t{}; s->stamps_pending = false; }
        s->profiling = enabled != 0;
    }
    return swh_success_k;
}
swh_status_t swh_scope_timing_totals(swh_scope_t handle, swh_timing_totals_t *totals) {
    if (!handle || !totals) return swh_invalid_argument_k;
    Scope *scope = (Scope *)handle;
    *totals = swh_timing_totals_t{};
    Scope *all[3] = {scope, scope->lanes[0], scope->lanes[1]};
    for (Scope *s : all) {
        if (!s) continue;
        totals->total_ms += s->totals.total_ms; totals->dominant_ms += s->totals.dominant_ms;
        totals->compute_ms += s->totals.compute_ms; totals->calls += s->totals.calls;
    }
    return swh_success_k;
}
swh_status_t swh_scope_last_timing(swh_scope_t handle, swh_timing_t *timing) {
    if (!handle || !timing) return swh_invalid_argument_k;
    *timing = ((Scope *)handle)->last_timing;
    return swh_success_k;
}

// ---- memory --------------------------------------------------------------------------------------
swh_status_t swh_unified_alloc(swh_scope_t handle, size_t bytes, void **pointer, const char **error) {
    if (!handle || !pointer) return fail(error, swh_invalid_argument_k, "null argument");
    (void)hipSetDevice(((Scope *)handle)->device);
    hipError_t err = hipHostMalloc(pointer, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocPortable);
    if (err != hipSuccess) return fail_hip(error, HipFailure{err, "hipHostMalloc"});
    return swh_success_k;
}
swh_status_t swh_unified_free(swh_scope_t, void *pointer) {
    if (pointer) (void)hipHostFree(pointer);
    return swh_success_k;
}
swh_status_t swh_device_alloc(swh_scope_t handle, size_t bytes, void **pointer, const char **error) {
    if (!handle || !pointer) return fail(error, swh_invalid_argument_k, "null argument");
    (void)hipSetDevice(((Scope *)handle)->device);
    hipError_t err = hipMalloc(pointer, bytes ? bytes : 1);
    if (err != hipSuccess) return fail_hip(error, HipFailure{err, "hipMalloc"});
    return swh_success_k;
}
swh_status_t swh_device_free(swh_scope_t, void *pointer) {
    if (pointer) (void)hipFree(pointer);
    return swh_success_k;
}
swh_status_t swh_copy_to_device(swh_scope_t handle, void *dst, const void *src, size_t bytes, const char **error) {
    Scope *scope = (Scope *)handle;
    if (!scope) return fail(error, swh_invalid_argument_k, "null scope");
    hipError_t err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, scope->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(scope->stream);
    if (err != hipSuccess) return fail_hip(error, HipFailure{err, "hipMemcpy H2D"});
    return swh_success_k;
}
swh_status_t swh_copy_to_host(swh_scope_t handle, void *dst, const void *src, size_t bytes, const char **error) {
    Scope *scope = (Scope *)handle;
    if (!scope) return fail(error, swh_invalid_argument_k, "null scope");
    hipError_t err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, scope->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(scope->stream);
    if (err != hipSuccess) return fail_hip(error, HipFailure{err, "hipMemcpy D2H"});
    return swh_success_k;
}

// ---- prepared tapes ----------------------------------------------------------------------------------
static void free_prepared(Prepared *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    for (void *buffer : p->owned) (void)hipFree(buffer);
    delete p;
}

static swh_status_t prepare_tape(Scope *scope, const HostTape &tape, bool utf8, swh_prepared_t *out, const char **error) {
    if (!scope || !out) return fail(error, swh_invalid_argument_k, "null argument");
    *out = nullptr;
    if (scope->pipelined) return fail(error, swh_invalid_argument_k, "prepare tapes before switching the scope to pipelined mode");
    Prepared *p = new Prepared();
    try {
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        p->device = scope->device;
        p->utf8 = utf8;
        p->off64 = (uint32_t)tape.off64;
        const size_t ow = tape.off64 ? 8 : 4;
        const bool dev_data = is_device_pointer(tape.data), dev_off = is_device_pointer(tape.offsets);
        p->total_bytes = tape.count || tape.offsets ? read_offset(tape.offsets, tape.off64, tape.count, dev_off, stream) : 0;
        auto own = [&](size_t bytes) -> void * {
            void *buffer = nullptr;
            SWH_HIP_CHECK(hipMalloc(&buffer, bytes ? bytes : 16));
            p->owned.push_back(buffer);
            return buffer;
        };
        // residency: host tapes are uploaded once (`BytesTape<u64, UnifiedAlloc>::extend`, bench.rs:292-301)
        const void *data = tape.data, *offsets = tape.offsets;
        if (!dev_data) {
            void *buffer = own(p->total_bytes + 16);
            if (p->total_bytes) SWH_HIP_CHECK(hipMemcpyAsync(buffer, tape.data, p->total_bytes, hipMemcpyHostToDevice, stream));
            data = buffer;
        }
        if (!dev_off) {
            void *buffer = own((tape.count + 1) * ow + 16);
            SWH_HIP_CHECK(hipMemcpyAsync(buffer, tape.offsets, (tape.count + 1) * ow, hipMemcpyHostToDevice, stream));
            offsets = buffer;
        }
        p->bytes = TapeRef{data, offsets, tape.count};
        // measurements: longest string in bytes (and in code points below)
        uint32_t *words = (uint32_t *)own((4 + kUtf8FlagWords) * sizeof(uint32_t));   // [0] longest bytes, [1] longest symbols, [4 ...] UTF-8 flag, balances, tickets
        SWH_HIP_CHECK(hipMemsetAsync(words, 0, (4 + kUtf8FlagWords) * sizeof(uint32_t), stream));
        launch_tape_longest(scope, offsets, p->off64, tape.count, words);
        uint64_t total_symbols = p->total_bytes;
        // offsets[0], for the mean string of a tape that is a window into a larger buffer (call_lengths): it travels with the words read
        // back below, under the synchronisation they need anyway
        uint64_t first_byte = 0;
        if (tape.count) {
            if (dev_off) SWH_HIP_CHECK(hipMemcpyAsync(&first_byte, tape.offsets, ow, hipMemcpyDeviceToHost, stream));
            else memcpy(&first_byte, tape.offsets, ow);
        }
        if (p->total_bytes >= kStringLimit) {
            // only such a tape can hold a string the windows cannot index (common.hpp: kStringLimit); it is refused on its offsets alone,
            // before anything is decoded -- in bytes, which bound the code points (k_tape_longest saturates at 2^32 - 1)
            uint32_t longest = 0;
            SWH_HIP_CHECK(hipMemcpyAsync(&longest, words, sizeof longest, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            if (longest >= kStringLimit) {
                free_prepared(p);
                return fail(error, swh_unsupported_length_k, "a string of %u bytes: one string holds fewer than 2^30", longest);
            }
        }
        if (utf8) {
            // validate + decode once: `CharsTapeView::try_from` (bench.rs:303-306)
            Utf8Args u{};
            u.in = p->bytes; u.off64 = p->off64; u.total_bytes = p->total_bytes; u.slot = 0;
            u.symbols = (uint32_t *)own((p->total_bytes + 4) * sizeof(uint32_t));
            u.offsets = (uint64_t *)own((tape.count + 1) * sizeof(uint64_t));
            void *scratch = nullptr;
            SWH_HIP_CHECK(hipMalloc(&scratch, utf8_scratch_words(p->total_bytes) * sizeof(uint32_t) + 256));
            u.counts = (uint32_t *)scratch;
            u.invalid = words + 4;
            hipError_t decode_error = hipSuccess;
            try { launch_utf8_decode(scope, u); } catch (const HipFailure &f) { decode_error = f.code; }
            launch_tape_longest(scope, u.offsets, 1, tape.count, words + 1);
            uint32_t host_words[8] = {0};
            SWH_HIP_CHECK(hipMemcpyAsync(host_words, words, sizeof host_words, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipMemcpyAsync(&total_symbols, u.offsets + tape.count, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            (void)hipFree(scratch);
            if (decode_error != hipSuccess) throw HipFailure{decode_error, "UTF-8 decode"};
            if (host_words[4]) {
                free_prepared(p);
                return fail(error, swh_invalid_utf8_k, "invalid UTF-8 in the tape (marker %u: a 4-byte word inside the 1 KiB tile that failed)", host_words[4] - 1);
            }
            p->longest_bytes = host_words[0];
            p->longest_symbols = host_words[1];
            p->symbols = TapeRef{u.symbols, u.offsets, tape.count};
            p->ascii = total_symbols == p->total_bytes;
        } else {
            uint32_t host_words[2] = {0, 0};
            SWH_HIP_CHECK(hipMemcpyAsync(host_words, words, sizeof host_words, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            p->longest_bytes = p->longest_symbols = host_words[0];
            p->symbols = p->bytes;
        }
        p->total_symbols = total_symbols;
        // (offsets that do not ascend are the caller's error and every kernel's reads stay clamped into the tape regardless; the mean only
        // sizes short.hip's chunks, so all it needs from such a tape is a difference that does not wrap)
        p->first_byte = std::min(first_byte, p->total_bytes);
        *out = (swh_prepared_t)p;
        return swh_success_k;
    } catch (const HipFailure &f) {
        free_prepared(p);
        return fail_hip(error, f);
    } catch (const std::bad_alloc &) {
        free_prepared(p);
        return fail(error, swh_bad_alloc_k, "host allocation failed");
    }
}

// ---- engines --------------------------------------------------------------------------------------
static swh_status_t upload_matrix(Engine *engine, const int8_t *matrix, const char **error) {
    hipError_t err = hipMalloc((void **)&engine->matrix_dev, 65536);
    if (err == hipSuccess) err = hipMemcpy(engine->matrix_dev, matrix, 65536, hipMemcpyHostToDevice);
    if (err != hipSuccess) return fail_hip(error, HipFailure{err, "substitution matrix upload"});
    engine->scoring.matrix = engine->matrix_dev;
    return swh_success_k;
}

swh_status_t swh_levenshtein_init(swh_scope_t handle, int match, int mismatch, int open, int extend,
                                  swh_levenshtein_t *out, const char **error) {
    if (!handle || !out) return fail(error, swh_invalid_argument_k, "null argument");
    if (match < 0 || mismatch < 0 || open < 0 || extend < 0 || match > 127 || mismatch > 127 || open > 4096 ||
        extend > 4096)
        return fail(error, swh_invalid_argument_k, "Levenshtein costs must be small non-negative integers");
    Scope *scope = (Scope *)handle;
    Engine *engine = new Engine{};
    engine->kind = 0;
    engine->device = scope->device;
    engine->unit_costs = match == 0 && mismatch == 1 && open == 1 && extend == 1;
    engine->algorithm = swh_algorithm_auto_k;
    // max-plus core: distances are negated scores
    engine->scoring = Scoring{-match, -mismatch, -open, -extend, nullptr, nullptr};
    // affine gaps (open != extend) run on the wavefront kernels' uniform-cost Gotoh model, bytes and code points alike
    *out = (swh_levenshtein_t)engine;
    return swh_success_k;
}
swh_status_t swh_levenshtein_free(swh_levenshtein_t handle) {
    Engine *engine = (Engine *)handle;
    if (!engine) return swh_success_k;
    if (engine->kind != 0 && engine->uid) drop_engine_clones(engine->uid);   // the per-device clones multi-device scopes made of it (sharded.hip)
    if (engine->matrix_dev) { (void)hipSetDevice(engine->device); (void)hipFree(engine->matrix_dev); }
    if (engine->class_dev) { (void)hipSetDevice(engine->device); (void)hipFree(engine->class_dev); }
    delete[] engine->matrix_host;
    delete engine;
    return swh_success_k;
}
swh_status_t swh_levenshtein_set_algorithm(swh_levenshtein_t handle, swh_algorithm_t algorithm) {
    if (!handle) return swh_invalid_argument_k;
    ((Engine *)handle)->algorithm = algorithm;
    return swh_success_k;
}

static uint64_t next_engine_uid() {
    static std::atomic<uint64_t> counter{1};
    return counter.fetch_add(1);
}
static swh_status_t alignment_init(int kind, swh_scope_t handle, const int8_t *matrix, int open, int extend, void **out,
                                   const char **error) {
    if (!handle || !out || !matrix) return fail(error, swh_invalid_argument_k, "null argument");
    if (open > 0 || extend > 0 || open < -4096 || extend < -4096)
        return fail(error, swh_invalid_argument_k, "gap costs must be in [-4096, 0]");
    Scope *scope = (Scope *)handle;
    Engine *engine = new Engine{};
    engine->kind = kind;
    engine->device = scope->device;
    engine->algorithm = swh_algorithm_wavefront_k;
    engine->scoring = Scoring{0, 0, open, extend, nullptr, nullptr};
    bool symmetric = true;
    for (int i = 0; i < 256 && symmetric; ++i)
        for (int j = 0; j < i; ++j)
            if (matrix[i * 256 + j] != matrix[j * 256 + i]) { symmetric = false; break; }
    engine->unit_costs = symmetric;  // reused as "columns may be swapped" for nw engines
    engine->matrix_host = new int8_t[65536];
    memcpy(engine->matrix_host, matrix, 65536);
    engine->uid = next_engine_uid();
    (void)hipSetDevice(scope->device);
    swh_status_t st = upload_matrix(engine, matrix, error);
    if (st != swh_success_k) { swh_levenshtein_free((swh_levenshtein_t)engine); return st; }   // (releases matrix_host, too)
    // Symbol classes: bytes whose matrix rows AND columns coincide are interchangeable. With <= 32 classes (the
    // reference's own byte_to_class + 32x32 model, bench.rs:95-108; also 20 amino acids + "other") the kernels keep a
    // 32-byte cost row in registers per step instead of one LDS lookup per cell.
    {
        constexpr int kMost = (int)kWideClasses;
        static thread_local uint8_t table[kMost * kMost + 256];
        uint8_t map[256];
        int rep[kMost], classes = 0;
        bool fits = true;
        for (int b = 0; b < 256 && fits; ++b) {
            int found = -1;
            for (int c = 0; c < classes && found < 0; ++c) {
                const int r = rep[c];
                bool same = memcmp(matrix + b * 256, matrix + r * 256, 256) == 0;
                for (int k = 0; k < 256 && same; ++k) same = matrix[k * 256 + b] == matrix[k * 256 + r];
                if (same) found = c;
            }
            if (found < 0) {
                if (classes == kMost) { fits = false; break; }
                rep[classes] = b; found = classes++;
            }
            map[b] = (uint8_t)found;
        }
        // Global alignment runs on scores relative to the all-gaps baseline (wavefront.hip): the table holds
        // cost - extend - open (= cost - 2 g for linear gaps; the affine kernel keeps H + (open - extend) in its strips and
        // takes the surplus back on the diagonal), which must still fit a signed byte (otherwise the 256x256 LDS path is used).
        const int bias = kind == 2 ? -open : -(extend + open);   // local alignment: no baseline to be relative to, but its strips hold H + open
        for (int i = 0; i < classes && fits; ++i)
            for (int j = 0; j < classes; ++j) {
                int v = (int)matrix[rep[i] * 256 + rep[j]] + bias;
                if (v < -128 || v > 127) { fits = false; break; }
            }
        if (fits) {
            // up to 32 classes: the register cost-row model every class kernel reads (rows of 32 bytes); 33 .. 128: rows of kWideClasses
            // bytes for the column-profile kernel alone (Scoring::wide_table)
            const bool wide = classes > 32;
            const int stride = wide ? kMost : 32;
            const size_t bytes = (size_t)stride * stride + 256;
            memset(table, 0, bytes);
            for (int i = 0; i < classes; ++i)
                for (int j = 0; j < classes; ++j) table[i * stride + j] = (uint8_t)(int8_t)((int)matrix[rep[i] * 256 + rep[j]] + bias);
            memcpy(table + (size_t)stride * stride, map, 256);
            hipError_t err = hipMalloc((void **)&engine->class_dev, bytes);
            if (err == hipSuccess) err = hipMemcpy(engine->class_dev, table, bytes, hipMemcpyHostToDevice);
            if (err != hipSuccess) { swh_levenshtein_free((swh_levenshtein_t)engine); return fail_hip(error, HipFailure{err, "class table upload"}); }
            if (wide) engine->scoring.wide_table = engine->class_dev;
            else engine->scoring.class_table = engine->class_dev;
            engine->scoring.classes = (uint32_t)classes;
            int widest = 0;   // of the costs themselves (not the biased table)
            for (int i = 0; i < classes; ++i)
                for (int j = 0; j < classes; ++j) widest = std::max(widest, std::abs((int)matrix[rep[i] * 256 + rep[j]]));
            engine->scoring.step_span = (uint32_t)(widest - open - extend);
        }
    }
    *out = engine;
    return swh_success_k;
}
}  // extern "C"
namespace swh {
swh_status_t clone_alignment_engine(const Engine *source, swh_scope_t scope, void **out, const char **error) {
    if (!source || source->kind == 0 || !source->matrix_host) return fail(error, swh_invalid_argument_k, "not an alignment engine");
    return alignment_init(source->kind, scope, source->matrix_host, source->scoring.open, source->scoring.extend, out, error);
}
}  // namespace swh
extern "C" {
static swh_status_t alignment_init_classes(int kind, swh_scope_t handle, const uint8_t *byte_to_class,
                                           const int8_t *class_costs, int open, int extend, void **out, const char **error) {
    if (!byte_to_class || !class_costs) return fail(error, swh_invalid_argument_k, "null argument");
    static thread_local int8_t table[65536];
    for (int i = 0; i < 256; ++i) {
        if (byte_to_class[i] >= 32) return fail(error, swh_invalid_argument_k, "byte_to_class entries must be < 32");
        for (int j = 0; j < 256; ++j) {
            if (byte_to_class[j] >= 32) return fail(error, swh_invalid_argument_k, "byte_to_class entries must be < 32");
            table[i * 256 + j] = class_costs[byte_to_class[i] * 32 + byte_to_class[j]];
        }
    }
    return alignment_init(kind, handle, table, open, extend, out, error);
}
swh_status_t swh_nw_init(swh_scope_t handle, const int8_t *matrix, int open, int extend, swh_nw_t *out, const char **error) {
    return alignment_init(1, handle, matrix, open, extend, (void **)out, error);
}
swh_status_t swh_nw_init_classes(swh_scope_t handle, const uint8_t *byte_to_class, const int8_t *class_costs, int open,
                                 int extend, swh_nw_t *out, const char **error) {
    return alignment_init_classes(1, handle, byte_to_class, class_costs, open, extend, (void **)out, error);
}
swh_status_t swh_nw_free(swh_nw_t handle) { return swh_levenshtein_free((swh_levenshtein_t)handle); }
swh_status_t swh_sw_init(swh_scope_t handle, const int8_t *matrix, int open, int extend, swh_sw_t *out, const char **error) {
    return alignment_init(2, handle, matrix, open, extend, (void **)out, error);
}
swh_status_t swh_sw_init_classes(swh_scope_t handle, const uint8_t *byte_to_class, const int8_t *class_costs, int open,
                                 int extend, swh_sw_t *out, const char **error) {
    return alignment_init_classes(2, handle, byte_to_class, class_costs, open, extend, (void **)out, error);
}
swh_status_t swh_sw_free(swh_sw_t handle) { return swh_levenshtein_free((swh_levenshtein_t)handle); }

// ---- calls -----------------------------------------------------------------------------------------
#define SWH_TAPE(t, w) HostTape{(t)->data, (const void *)(t)->offsets, (t)->count, (w)}

static swh_status_t lev_pairs(swh_levenshtein_t e, swh_scope_t s, HostTape a, HostTape b, bool utf8, uint32_t bound,
                              uint32_t *out, size_t stride, const char **error) {
    if (e && ((Engine *)e)->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    CallSpec spec{a, b, false, utf8, bound, out, stride ? stride : 4, 0, false};
    if (spec.out_stride < 4) return fail(error, swh_invalid_argument_k, "out_stride_bytes must be >= 4");
    return run_call((Scope *)s, (Engine *)e, spec, error);
}

swh_status_t swh_levenshtein_pairs_u32tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u32_t *a,
                                           const swh_tape_u32_t *b, uint32_t bound, uint32_t *out, size_t stride,
                                           const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    return lev_pairs(e, s, SWH_TAPE(a, 0), SWH_TAPE(b, 0), false, bound, out, stride, error);
}
swh_status_t swh_levenshtein_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a,
                                           const swh_tape_u64_t *b, uint32_t bound, uint32_t *out, size_t stride,
                                           const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    return lev_pairs(e, s, SWH_TAPE(a, 1), SWH_TAPE(b, 1), false, bound, out, stride, error);
}
swh_status_t swh_levenshtein_utf8_pairs_u32tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u32_t *a,
                                                const swh_tape_u32_t *b, uint32_t bound, uint32_t *out, size_t stride,
                                                const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    return lev_pairs(e, s, SWH_TAPE(a, 0), SWH_TAPE(b, 0), true, bound, out, stride, error);
}
swh_status_t swh_levenshtein_utf8_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a,
                                                const swh_tape_u64_t *b, uint32_t bound, uint32_t *out, size_t stride,
                                                const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    return lev_pairs(e, s, SWH_TAPE(a, 1), SWH_TAPE(b, 1), true, bound, out, stride, error);
}

static swh_status_t cross_call(void *e, int kind, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                               bool utf8, void *out, size_t row_stride, const char **error) {
    if (!a) return fail(error, swh_invalid_argument_k, "null tape");
    if (e && ((Engine *)e)->kind != kind) return fail(error, swh_invalid_argument_k, "engine kind mismatch");
    const swh_tape_u64_t *bb = b ? b : a;
    CallSpec spec{SWH_TAPE(a, 1), SWH_TAPE(bb, 1), true, utf8, SWH_UNBOUNDED, out, 8,
                  row_stride ? row_stride : bb->count * 8, true};
    if (spec.row_stride < bb->count * 8) return fail(error, swh_invalid_argument_k, "row_stride_bytes too small");
    return run_call((Scope *)s, (Engine *)e, spec, error);
}
swh_status_t swh_levenshtein_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a,
                                           const swh_tape_u64_t *b, size_t *out, size_t row_stride, const char **error) {
    return cross_call(e, 0, s, a, b, false, out, row_stride, error);
}
swh_status_t swh_levenshtein_utf8_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a,
                                                const swh_tape_u64_t *b, size_t *out, size_t row_stride,
                                                const char **error) {
    return cross_call(e, 0, s, a, b, true, out, row_stride, error);
}
swh_status_t swh_nw_cross_u64tape(swh_nw_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                  ptrdiff_t *out, size_t row_stride, const char **error) {
    return cross_call(e, 1, s, a, b, false, out, row_stride, error);
}

static swh_status_t nw_pairs(void *e, int kind, swh_scope_t s, HostTape a, HostTape b, int32_t *out, size_t stride,
                             const char **error) {
    if (e && ((Engine *)e)->kind != kind) return fail(error, swh_invalid_argument_k, "engine kind mismatch");
    CallSpec spec{a, b, false, false, SWH_UNBOUNDED, out, stride ? stride : 4, 0, false};
    if (spec.out_stride < 4) return fail(error, swh_invalid_argument_k, "out_stride_bytes must be >= 4");
    return run_call((Scope *)s, (Engine *)e, spec, error);
}
swh_status_t swh_nw_pairs_u32tape(swh_nw_t e, swh_scope_t s, const swh_tape_u32_t *a, const swh_tape_u32_t *b,
                                  int32_t *out, size_t stride, const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    return nw_pairs(e, 1, s, SWH_TAPE(a, 0), SWH_TAPE(b, 0), out, stride, error);
}
swh_status_t swh_nw_pairs_u64tape(swh_nw_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                  int32_t *out, size_t stride, const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    return nw_pairs(e, 1, s, SWH_TAPE(a, 1), SWH_TAPE(b, 1), out, stride, error);
}

swh_status_t swh_sw_pairs_u32tape(swh_sw_t e, swh_scope_t s, const swh_tape_u32_t *a, const swh_tape_u32_t *b,
                                  int32_t *out, size_t stride, const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    return nw_pairs(e, 2, s, SWH_TAPE(a, 0), SWH_TAPE(b, 0), out, stride, error);
}
swh_status_t swh_sw_pairs_u64tape(swh_sw_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                  int32_t *out, size_t stride, const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    return nw_pairs(e, 2, s, SWH_TAPE(a, 1), SWH_TAPE(b, 1), out, stride, error);
}
swh_status_t swh_sw_cross_u64tape(swh_sw_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                  ptrdiff_t *out, size_t row_stride, const char **error) {
    return cross_call(e, 2, s, a, b, false, out, row_stride, error);
}

// ---- prepared tapes and the calls on them ------------------------------------------------------------------
swh_status_t swh_tape_prepare_u32(swh_scope_t scope, const swh_tape_u32_t *tape, int utf8, swh_prepared_t *prepared, const char **error) {
    if (!tape) return fail(error, swh_invalid_argument_k, "null tape");
    return prepare_tape((Scope *)scope, SWH_TAPE(tape, 0), utf8 != 0, prepared, error);
}
swh_status_t swh_tape_prepare_u64(swh_scope_t scope, const swh_tape_u64_t *tape, int utf8, swh_prepared_t *prepared, const char **error) {
    if (!tape) return fail(error, swh_invalid_argument_k, "null tape");
    return prepare_tape((Scope *)scope, SWH_TAPE(tape, 1), utf8 != 0, prepared, error);
}
swh_status_t swh_prepared_info(swh_prepared_t handle, swh_prepared_info_t *info) {
    const Prepared *p = (const Prepared *)handle;
    if (!p || !info) return swh_invalid_argument_k;
    info->count = (size_t)p->bytes.count;
    info->bytes = p->total_bytes;
    info->symbols = p->total_symbols;
    info->longest = p->utf8 ? p->longest_symbols : p->longest_bytes;
    info->utf8 = p->utf8 ? 1 : 0;
    info->ascii = p->ascii ? 1 : 0;
    return swh_success_k;
}
swh_status_t swh_prepared_free(swh_prepared_t handle) {
    free_prepared((Prepared *)handle);
    return swh_success_k;
}

static swh_status_t prepared_call(void *e, int kind, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                  bool cross, uint32_t bound, void *out, size_t stride, const char **error) {
    if (!a || !a->tape) return fail(error, swh_invalid_argument_k, "null prepared view");
    if (e && ((Engine *)e)->kind != kind) return fail(error, swh_invalid_argument_k, "engine kind mismatch");
    const swh_prepared_view_t *bb = (b && b->tape) ? b : (cross ? a : nullptr);
    if (!bb) return fail(error, swh_invalid_argument_k, "null prepared view");
    if (!view_fits(a) || !view_fits(bb)) return fail(error, swh_invalid_argument_k, "view exceeds the prepared tape");
    const Prepared *pa = (const Prepared *)a->tape, *pb = (const Prepared *)bb->tape;
    CallSpec spec{};
    spec.a = HostTape{nullptr, nullptr, a->count, 0};
    spec.b = HostTape{nullptr, nullptr, bb->count, 0};
    spec.cross = cross; spec.utf8 = pa->utf8; spec.bound = bound; spec.out = out;
    if (cross) {
        spec.out_stride = 8; spec.out64 = true;
        spec.row_stride = stride ? stride : bb->count * 8;
        if (spec.row_stride < bb->count * 8) return fail(error, swh_invalid_argument_k, "row_stride_bytes too small");
    } else {
        spec.out_stride = stride ? stride : 4; spec.out64 = false;
        if (spec.out_stride < 4) return fail(error, swh_invalid_argument_k, "out_stride_bytes must be >= 4");
    }
    spec.pa = pa; spec.pb = pb; spec.a_first = a->first; spec.b_first = bb->first;
    return run_call((Scope *)s, (Engine *)e, spec, error);
}
swh_status_t swh_levenshtein_pairs_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                            uint32_t bound, uint32_t *out, size_t stride, const char **error) {
    return prepared_call(e, 0, s, a, b, false, bound, out, stride, error);
}
swh_status_t swh_levenshtein_cross_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                            size_t *out, size_t row_stride, const char **error) {
    return prepared_call(e, 0, s, a, b, true, SWH_UNBOUNDED, out, row_stride, error);
}
swh_status_t swh_nw_pairs_prepared(swh_nw_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b, int32_t *out,
                                   size_t stride, const char **error) {
    return prepared_call(e, 1, s, a, b, false, SWH_UNBOUNDED, out, stride, error);
}
swh_status_t swh_nw_cross_prepared(swh_nw_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b, ptrdiff_t *out,
                                   size_t row_stride, const char **error) {
    return prepared_call(e, 1, s, a, b, true, SWH_UNBOUNDED, out, row_stride, error);
}
swh_status_t swh_sw_pairs_prepared(swh_sw_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b, int32_t *out,
                                   size_t stride, const char **error) {
    return prepared_call(e, 2, s, a, b, false, SWH_UNBOUNDED, out, stride, error);
}
swh_status_t swh_sw_cross_prepared(swh_sw_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b, ptrdiff_t *out,
                                   size_t row_stride, const char **error) {
    return prepared_call(e, 2, s, a, b, true, SWH_UNBOUNDED, out, row_stride, error);
}

}  // extern "C"

// ---- the synchronous two-tape calls: one front end ------------------------------------------------------------------------------------
// Top-k and range searches, alignments, infix search and the scored families (OSA, LCS, Jaro) are synchronous on every scope:
// outstanding asynchronous / pipelined work is joined first, and the call runs on the scope itself (not on a pipeline lane) with the
// asynchronous mode held off until it returns. Every export runs its own null tests and argument checks in its own order -- which
// refusal wins is its contract (DESIGN.md lists where the calls differ on purpose) -- and between them resolves its two sides here,
// into the TapePair its *_run takes.
struct TapePair {
    const Prepared *pa = nullptr, *pb = nullptr;   // null where a raw call prepared nothing: every *_run returns before it looks at them
    size_t a_first = 0, a_count = 0, b_first = 0, b_count = 0;
};
struct PreparedOwner {
    Prepared *p = nullptr;
    ~PreparedOwner() { free_prepared(p); }
};
static swh_status_t join_outstanding(Scope *scope, const char **error) {
    if (!scope->async && !scope->pipelined) return swh_success_k;
    return swh_scope_synchronize((swh_scope_t)scope, error);
}

struct HoldSynchronous {
    Scope *scope = nullptr;
    bool async = false, pipelined = false;
    void hold(Scope *s) { scope = s; async = s->async; pipelined = s->pipelined; s->async = false; s->pipelined = false; }
    ~HoldSynchronous() {
        if (scope) { scope->async = async; scope->pipelined = pipelined; }
    }
};
struct TwoTapeCall {
    HoldSynchronous mode;             // declared first, so the scope's mode comes back last: after what the call prepared is freed
    Scope *scope = nullptr;           // set once the call has begun
    PreparedOwner owned_a, owned_b;   // what a raw call prepared: it lives as long as the call
    TapePair pair;

    // joins what is outstanding and holds the scope synchronous until the call returns
    swh_status_t begin(swh_scope_t s, const char **error) {
        const swh_status_t status = join_outstanding((Scope *)s, error);
        if (status != swh_success_k) return status;
        scope = (Scope *)s;
        mode.hold(scope);
        return swh_success_k;
    }
    // Raw tapes, after begin(): the sides named are made resident and measured for the call (prepare_tape: device tapes in place, host
    // tapes uploaded; UTF-8 validated and decoded), so the route is chosen on lengths that are known, not believed. Without `b` the
    // second side is the first. A call without pairs names no side: its pair keeps the counts and null tapes.
    swh_status_t prepare(const swh_tape_u64_t *a, const swh_tape_u64_t *b, bool utf8, bool prepare_a, bool prepare_b, const char **error) {
        pair = TapePair{nullptr, nullptr, 0, a->count, 0, (b ? b : a)->count};
        swh_status_t status = swh_success_k;
        if (prepare_a && (status = prepare_tape(scope, SWH_TAPE(a, 1), utf8, (swh_prepared_t *)&owned_a.p, error)) != swh_success_k) return status;
        if (b && prepare_b && (status = prepare_tape(scope, SWH_TAPE(b, 1), utf8, (swh_prepared_t *)&owned_b.p, error)) != swh_success_k) return status;
        pair.pa = owned_a.p; pair.pb = b ? owned_b.p : owned_a.p;
        return swh_success_k;
    }
    // Prepared views, before the call's own checks: the null tests and the bounds of both. A missing b is a (the self-search, the
    // self-product) where `b_optional`.
    swh_status_t views(const swh_prepared_view_t *a, const swh_prepared_view_t *b, bool b_optional, const char **error) {
        if (!a || !a->tape) return fail(error, swh_invalid_argument_k, "null prepared view");
        const swh_prepared_view_t *bb = (b && b->tape) ? b : (b_optional ? a : nullptr);
        if (!bb) return fail(error, swh_invalid_argument_k, "null prepared view");
        if (!view_fits(a) || !view_fits(bb)) return fail(error, swh_invalid_argument_k, "view exceeds the prepared tape");
        pair = TapePair{(const Prepared *)a->tape, (const Prepared *)bb->tape, a->first, a->count, bb->first, bb->count};
        return swh_success_k;
    }
    // ... and after them: the two tapes go together and live on the scope's device, and the call begins
    swh_status_t begin_on_views(swh_scope_t s, const char **error) {
        const swh_status_t status = check_prepared_pair((Scope *)s, pair.pa, pair.pb, error);
        return status != swh_success_k ? status : begin(s, error);
    }
};

// What every *_run is wrapped in: the previous call's timing is harvested and this call's begins empty; a HIP or allocation failure
// anywhere in `body` becomes the call's status.
template <typename Body> static swh_status_t synchronous_run(Scope *scope, const char **error, Body body) {
    harvest_timing(scope, false);
    scope->stamps_used = 0;
    scope->last_timing = swh_timing_t{};
    try {
        return body();
    } catch (const HipFailure &f) {
        return fail_hip(error, f);
    } catch (const std::bad_alloc &) {
        return fail(error, swh_bad_alloc_k, "host allocation failed");
    }
}

// ---- the search planner: what top-k and the range search decide alike ---------------------------------------------------------------
// Both searches run word-sized byte strings on unit costs through a fused kernel of their own (k_cross_topk, k_cross_within): the
// searches a dense cross-product of the same views would run on k_cross_short (pick_route for prepared tapes). Everything else takes
// the general path: the candidates in slices, each slice scored by the ordinary cross-product routes into a u32 matrix in scratch
// (with the caller's bound, so long strings may take the banded kernel) and handed to the search's own kernels. What differs between
// the two comes in as a value or a callback.
// `force_select`: the search's STRINGWARS_AMD_*_ROUTE=select hook; `dev_out`: its results go to device memory
static bool search_is_fused(const Scope *scope, const Engine *engine, const TapePair &p, uint32_t bound, bool force_select, bool dev_out) {
    const bool utf8 = p.pa->utf8 && !(p.pa->ascii && p.pb->ascii && p.pa->off64 == p.pb->off64);
    CallSpec whole{};   // the dense cross-product of the two views, as run_call_on would route it
    whole.a.count = p.a_count; whole.b.count = p.b_count; whole.cross = true; whole.bound = bound; whole.pa = p.pa; whole.pb = p.pb;
    return !force_select && !utf8 && engine->algorithm == swh_algorithm_auto_k && p.pa->off64 == p.pb->off64 &&
           pick_route(scope, engine, whole, false, dev_out, call_lengths(scope, engine, whole, false)).route == kRouteCrossShort;
}

// The fused kernels' candidate slices per block of 16 queries: enough for ~32 items per compute unit (a few rounds of its 12 wave
// slots: 65 536 x 1 M words ran top-k at 4.6 TCUPS with 16, 5.9 with 32), while what the search keeps per (row, slice) --
// `row_slice_bytes` -- stays under 256 MB; at most one per chunk of 64 candidates. `forced`: a test hook's count, 0 without one.
struct SearchSlices { uint64_t slices, slice_chunks; };
static SearchSlices search_slices(uint64_t nq, uint64_t nc, uint64_t compute_units, uint64_t row_slice_bytes, uint64_t forced) {
    const uint64_t qblocks = (nq + 15) / 16, chunks = (nc + 63) / 64;
    const uint64_t target = compute_units * 32;
    uint64_t slices = std::min<uint64_t>(std::max<uint64_t>((target + qblocks - 1) / qblocks, 1), chunks);
    slices = std::max<uint64_t>(1, std::min<uint64_t>(slices, ((uint64_t)256 << 20) / (nq * row_slice_bytes)));
    if (forced) slices = std::min<uint64_t>(forced, chunks);
    const uint64_t slice_chunks = (chunks + slices - 1) / slices;
    return SearchSlices{(chunks + slice_chunks - 1) / slice_chunks, slice_chunks};
}

// The general path: query blocks of at most 2^18 rows x candidate slices of at most 2^26 pairs (a 256 MB u32 matrix), and the search
// reported as one call whose name says which path ran and which kernel scored the pairs.
struct SearchSweep {
    Scope *scope; const Engine *engine; const TapePair &pair; uint32_t bound;
    uint64_t q_step, c_step;
    swh_timing_totals_t totals_before;
    swh_timing_t sum{};
    char scoring_name[64] = "";

    SearchSweep(Scope *s, const Engine *e, const TapePair &p, uint32_t bound_)
        : scope(s), engine(e), pair(p), bound(bound_), q_step(std::min<uint64_t>(p.a_count, (uint64_t)1 << 18)),
          c_step(std::max<uint64_t>(1, std::min<uint64_t>(p.b_count, ((uint64_t)1 << 26) / q_step))), totals_before(s->totals) {}

    // One walk over the blocks. rows_begin(q0, rows) opens every block of queries, before its first slice is scored; each slice is then
    // scored into `matrix` (q_step * c_step entries) and handed to block(q0, rows, c0, columns, last_slice) with the stamps reset.
    // `counted`: the walk's cells and bytes go into the sum (a second walk of the same pairs: not again).
    template <typename Rows, typename Block>
    swh_status_t walk(uint32_t *matrix, bool counted, const char **error, Rows rows_begin, Block block) {
        const uint64_t nq = pair.a_count, nc = pair.b_count;
        for (uint64_t q0 = 0; q0 < nq; q0 += q_step) {
            const uint64_t rows = std::min<uint64_t>(q_step, nq - q0);
            rows_begin(q0, rows);
            for (uint64_t c0 = 0; c0 < nc; c0 += c_step) {
                const uint64_t columns = std::min<uint64_t>(c_step, nc - c0);
                CallSpec spec{};
                spec.a = HostTape{nullptr, nullptr, (size_t)rows, 0};
                spec.b = HostTape{nullptr, nullptr, (size_t)columns, 0};
                spec.cross = true; spec.utf8 = pair.pa->utf8; spec.bound = bound;
                spec.out = matrix; spec.out_stride = 4; spec.row_stride = columns * 4; spec.out64 = false;
                spec.pa = pair.pa; spec.pb = pair.pb; spec.a_first = pair.a_first + q0; spec.b_first = pair.b_first + c0;
                const swh_status_t status = run_call_on(scope, engine, spec, error);
                if (status != swh_success_k) return status;
                const swh_timing_t &dp = scope->last_timing;
                if (counted) { sum.cells += dp.cells; sum.bytes += dp.bytes; }
                sum.total_ms += dp.total_ms; sum.compute_ms += dp.compute_ms; sum.kernels += dp.kernels;
                if (dp.dominant_ms > sum.dominant_ms) { sum.dominant_ms = dp.dominant_ms; snprintf(scoring_name, sizeof scoring_name, "%s", dp.dominant_name); }
                scope->stamps_used = 0;
                scope->stamps_pending = false;
                block(q0, rows, c0, columns, c0 + columns == nc);
            }
        }
        return swh_success_k;
    }
    // with profiling on, the time of the `launched` kernels of the search's own since the last scoring call
    void time_own_kernels(uint32_t launched) {
        if (!scope->profiling) return;
        SWH_HIP_CHECK(hipStreamSynchronize(scope->stream));
        collect_timing(scope);
        sum.total_ms += scope->last_timing.total_ms; sum.compute_ms += scope->last_timing.compute_ms; sum.kernels += launched;
        scope->stamps_used = 0;
    }
    // the search as one call, "<search>_select/<scoring kernel>", once in the scope's totals
    void close(const char *search) {
        scope->summary_pending = false;
        scope->stamps_pending = false;
        snprintf(sum.dominant_name, sizeof sum.dominant_name, "%s_select/%s", search, scoring_name);
        scope->last_timing = sum;
        if (scope->profiling) {
            scope->totals = totals_before;
            add_to_totals(scope->totals, sum);
        }
    }
};

extern "C" {
// ---- top-k search (topk.hip) ----------------------------------------------------------------------------------------------------------
// The fused kernel keeps a list of k per (row, slice) and merges them; the general path folds each scored slice into the running
// lists with k_topk_select.
// STRINGWARS_AMD_TOPK_PRUNE=0 (test library): the fused kernel walks every chunk, also those the length bound rules out (the comparison knob)
static uint32_t topk_prune() {
    static const uint32_t on = [] { const char *e = test_hook("STRINGWARS_AMD_TOPK_PRUNE"); return !e || atoi(e) != 0 ? 1u : 0u; }();
    return on;
}
// STRINGWARS_AMD_TOPK_ROUTE=select (test library): every search on the general path
static bool topk_force_select() {
    static const bool on = [] { const char *e = test_hook("STRINGWARS_AMD_TOPK_ROUTE"); return e && !strcmp(e, "select"); }();
    return on;
}

static swh_status_t topk_run(Scope *scope, const Engine *engine, const TapePair &p, uint32_t k32, uint32_t bound, uint32_t *indices,
                             uint32_t *distances, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t nq = p.a_count, nc = p.b_count, k = k32;
        if (nq == 0) return swh_success_k;
        const uint64_t cap = bound == SWH_UNBOUNDED ? ~0ull : ((uint64_t)bound + 1) << 32;
        const size_t out_bytes = nq * k * sizeof(uint32_t);
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        const bool dev_i = is_device_pointer(indices), dev_d = is_device_pointer(distances);
        if (nc == 0) {   // every row is padding
            if (dev_i) SWH_HIP_CHECK(hipMemsetAsync(indices, 0xFF, out_bytes, stream)); else memset(indices, 0xFF, out_bytes);
            if (dev_d) SWH_HIP_CHECK(hipMemsetAsync(distances, 0xFF, out_bytes, stream)); else memset(distances, 0xFF, out_bytes);
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            return swh_success_k;
        }
        const size_t ow = p.pa->off64 ? 8 : 4;
        auto finish_outputs = [&](uint32_t *ind, uint32_t *dist) {
            if (!dev_i) SWH_HIP_CHECK(hipMemcpyAsync(indices, ind, out_bytes, hipMemcpyDeviceToHost, stream));
            if (!dev_d) SWH_HIP_CHECK(hipMemcpyAsync(distances, dist, out_bytes, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
        };

        if (search_is_fused(scope, engine, p, bound, topk_force_select(), dev_i)) {
            // ---- fused: a partial list of k (index, distance) words per (row, slice) ------------------------------------------------------
            const SearchSlices cut = search_slices(nq, nc, scope->compute_units, k * 8, 0);
            const uint64_t slices = cut.slices;
            const size_t need = (slices > 1 ? pad(nq * slices * k * 8) : 0) + (dev_i ? 0 : pad(out_bytes)) + (dev_d ? 0 : pad(out_bytes));
            ensure(scope->topk_scratch, scope->topk_scratch_bytes, need);
            Carver sc{scope->topk_scratch, 0, scope->topk_scratch_bytes};
            TopkLaunch t{};
            t.a = prepared_view(p.pa, false, p.a_first, nq); t.b = prepared_view(p.pb, false, p.b_first, nc);
            t.off64 = p.pa->off64; t.k = (uint32_t)k; t.slices = (uint32_t)slices; t.prune = topk_prune();
            t.slice_chunks = cut.slice_chunks; t.cap = cap;
            t.partial = slices > 1 ? sc.take<uint64_t>(nq * slices * k) : nullptr;
            t.indices = dev_i ? indices : sc.take<uint32_t>(nq * k);
            t.distances = dev_d ? distances : sc.take<uint32_t>(nq * k);
            scope->summary_slot = 0;
            launch_cross_topk(scope, t);
            finish_outputs(t.indices, t.distances);
            const CallSummary sm = scope->summary_host[0];
            if (!sm.violation) {
                if (scope->profiling && scope->stamps_used) {
                    collect_timing(scope);
                    add_to_totals(scope->totals, scope->last_timing);
                }
                scope->last_timing.cells = sm.cells;
                scope->last_timing.bytes = p.pa->total_bytes + p.pb->total_bytes + (nq + nc) * ow + 2 * out_bytes;
                return swh_success_k;
            }
            // a string longer than the kernel takes (the memory of a prepared tape changed since it was measured): the general path
            scope->stamps_used = 0;
            scope->last_timing = swh_timing_t{};
        }

        // ---- general path: each slice folded into the block's running lists ---------------------------------------------------------------
        SearchSweep sweep(scope, engine, p, bound);
        const size_t need = pad(sweep.q_step * sweep.c_step * 4) + pad(sweep.q_step * k * 8) + (dev_i ? 0 : pad(out_bytes)) + (dev_d ? 0 : pad(out_bytes));
        ensure(scope->topk_scratch, scope->topk_scratch_bytes, need);
        Carver sc{scope->topk_scratch, 0, scope->topk_scratch_bytes};
        uint32_t *matrix = sc.take<uint32_t>(sweep.q_step * sweep.c_step);
        uint64_t *lists = sc.take<uint64_t>(sweep.q_step * k);
        uint32_t *ind = dev_i ? indices : sc.take<uint32_t>(nq * k);
        uint32_t *dist = dev_d ? distances : sc.take<uint32_t>(nq * k);
        auto pad_lists = [&](uint64_t, uint64_t rows) { SWH_HIP_CHECK(hipMemsetAsync(lists, 0xFF, rows * k * 8, stream)); };   // every row is padding
        const swh_status_t status = sweep.walk(matrix, true, error, pad_lists, [&](uint64_t q0, uint64_t rows, uint64_t c0, uint64_t columns, bool last_slice) {
            launch_topk_select(scope, matrix, rows, columns, q0, c0, (uint32_t)k, cap, lists, last_slice, ind, dist);
            sweep.time_own_kernels(1);
        });
        if (status != swh_success_k) return status;
        finish_outputs(ind, dist);
        sweep.close("topk");
        return swh_success_k;
    });
}

static swh_status_t topk_checks(swh_levenshtein_t e, swh_scope_t s, size_t k, size_t queries, size_t candidates, const uint32_t *indices,
                                const uint32_t *distances, const char **error) {
    if (!s || !e) return fail(error, swh_invalid_argument_k, "null scope or engine");
    if (((Engine *)e)->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (k < 1 || k > SWH_TOPK_MAX) return fail(error, swh_invalid_argument_k, "k must lie in [1, SWH_TOPK_MAX]");
    if (candidates >= 0xFFFFFFFFull) return fail(error, swh_unsupported_length_k, "2^32 - 1 candidates or more");
    if (queries && (!indices || !distances)) return fail(error, swh_invalid_argument_k, "null output pointer");
    return swh_success_k;
}

static swh_status_t topk_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *q, const swh_tape_u64_t *c, bool utf8, size_t k,
                               uint32_t bound, uint32_t *indices, uint32_t *distances, const char **error) {
    if (!q) return fail(error, swh_invalid_argument_k, "null tape");
    swh_status_t status = topk_checks(e, s, k, q->count, (c ? c : q)->count, indices, distances, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    if (q->count == 0) return swh_success_k;
    if ((status = call.prepare(q, c, utf8, true, true, error)) != swh_success_k) return status;
    return topk_run(call.scope, (Engine *)e, call.pair, (uint32_t)k, bound, indices, distances, error);
}
swh_status_t swh_levenshtein_topk_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries, const swh_tape_u64_t *candidates,
                                          size_t k, uint32_t bound, uint32_t *indices, uint32_t *distances, const char **error) {
    return topk_tapes(e, s, queries, candidates, false, k, bound, indices, distances, error);
}
swh_status_t swh_levenshtein_utf8_topk_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries,
                                               const swh_tape_u64_t *candidates, size_t k, uint32_t bound, uint32_t *indices,
                                               uint32_t *distances, const char **error) {
    return topk_tapes(e, s, queries, candidates, true, k, bound, indices, distances, error);
}
swh_status_t swh_levenshtein_topk_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *queries,
                                           const swh_prepared_view_t *candidates, size_t k, uint32_t bound, uint32_t *indices,
                                           uint32_t *distances, const char **error) {
    TwoTapeCall call;
    swh_status_t status = call.views(queries, candidates, true, error);
    if (status != swh_success_k) return status;
    if ((status = topk_checks(e, s, k, call.pair.a_count, call.pair.b_count, indices, distances, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return topk_run(call.scope, (Engine *)e, call.pair, (uint32_t)k, bound, indices, distances, error);
}

// ---- range search (within.hip) ---------------------------------------------------------------------------------------------------------
// Every candidate within `bound` of every query, as CSR, on the search planner's routes. Both count first, scan the counts into the row
// offsets on the device, read the total (8 bytes) and fill only if the caller's arrays hold it.
// STRINGWARS_AMD_WITHIN_PRUNE=0 (test library): the fused kernel walks every chunk, also those the length gap rules out
static uint32_t within_prune() {
    static const uint32_t on = [] { const char *e = test_hook("STRINGWARS_AMD_WITHIN_PRUNE"); return !e || atoi(e) != 0 ? 1u : 0u; }();
    return on;
}
// STRINGWARS_AMD_WITHIN_ROUTE=select (test library): every search on the general path
static bool within_force_select() {
    static const bool on = [] { const char *e = test_hook("STRINGWARS_AMD_WITHIN_ROUTE"); return e && !strcmp(e, "select"); }();
    return on;
}
// STRINGWARS_AMD_WITHIN_SLICES=n (test library): the fused kernel's candidate slices per query block (at most one per chunk)
static uint64_t within_slices_hook() {
    static const uint64_t n = [] { const char *e = test_hook("STRINGWARS_AMD_WITHIN_SLICES"); return e && atoll(e) > 0 ? (uint64_t)atoll(e) : 0; }();
    return n;
}

struct WithinOutputs {
    size_t *row_offsets;
    uint32_t *indices, *distances;
    size_t capacity;
};

static swh_status_t within_run(Scope *scope, const Engine *engine, const TapePair &p, uint32_t bound, const WithinOutputs &r, const char **error) {
    static_assert(sizeof(size_t) == sizeof(uint64_t), "row offsets are scanned as 64-bit words");
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t nq = p.a_count, nc = p.b_count;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        const bool dev_o = is_device_pointer(r.row_offsets), dev_i = is_device_pointer(r.indices), dev_d = is_device_pointer(r.distances);
        if (nq == 0 || nc == 0) {   // no row, or every row empty
            const size_t bytes = (nq + 1) * sizeof(size_t);
            if (dev_o) {
                SWH_HIP_CHECK(hipMemsetAsync(r.row_offsets, 0, bytes, stream));
                SWH_HIP_CHECK(hipStreamSynchronize(stream));
            } else {
                memset(r.row_offsets, 0, bytes);
            }
            return swh_success_k;
        }
        const size_t ow = p.pa->off64 ? 8 : 4;
        // the offsets are complete on the device: the total decides the fill, the rest goes to a host caller
        auto read_total = [&](const uint64_t *offs) {
            uint64_t total = 0;
            SWH_HIP_CHECK(hipMemcpyAsync(&total, offs + nq, sizeof total, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            return total;
        };
        auto finish_offsets = [&](const uint64_t *offs) {
            if (!dev_o) SWH_HIP_CHECK(hipMemcpyAsync(r.row_offsets, offs, (nq + 1) * sizeof(size_t), hipMemcpyDeviceToHost, stream));
        };
        // where the fill pass writes: the caller's device arrays, or staging for its host arrays
        uint32_t *ind = nullptr, *dist = nullptr;
        auto stage_outputs = [&](uint64_t total) {
            const size_t need = (dev_i ? 0 : pad(total * 4)) + (dev_d ? 0 : pad(total * 4));
            ensure(scope->within_out, scope->within_out_bytes, need);
            Carver oc{scope->within_out, 0, scope->within_out_bytes};
            ind = dev_i ? r.indices : oc.take<uint32_t>(total);
            dist = dev_d ? r.distances : oc.take<uint32_t>(total);
        };
        auto finish_outputs = [&](uint64_t total) {
            if (!dev_i) SWH_HIP_CHECK(hipMemcpyAsync(r.indices, ind, total * 4, hipMemcpyDeviceToHost, stream));
            if (!dev_d) SWH_HIP_CHECK(hipMemcpyAsync(r.distances, dist, total * 4, hipMemcpyDeviceToHost, stream));
        };

        if (search_is_fused(scope, engine, p, bound, within_force_select(), dev_i)) {
            // ---- fused: a count (4 bytes) and a start (8) per (row, slice) ----------------------------------------------------------------
            const SearchSlices cut = search_slices(nq, nc, scope->compute_units, 12, within_slices_hook());
            const uint64_t slices = cut.slices;
            const uint64_t n_counts = nq * slices, tiles = (n_counts + kWithinScanTile - 1) / kWithinScanTile;
            const size_t need = pad(n_counts * 4) + pad(n_counts * 8) + pad(tiles * 8) + (dev_o ? 0 : pad((nq + 1) * 8));
            ensure(scope->topk_scratch, scope->topk_scratch_bytes, need);
            Carver sc{scope->topk_scratch, 0, scope->topk_scratch_bytes};
            WithinLaunch w{};
            w.a = prepared_view(p.pa, false, p.a_first, nq); w.b = prepared_view(p.pb, false, p.b_first, nc);
            w.off64 = p.pa->off64; w.slices = (uint32_t)slices; w.bound = bound; w.prune = within_prune(); w.slice_chunks = cut.slice_chunks;
            w.counts = sc.take<uint32_t>(n_counts);
            uint64_t *starts = sc.take<uint64_t>(n_counts), *block_sums = sc.take<uint64_t>(tiles);
            uint64_t *offs = dev_o ? (uint64_t *)r.row_offsets : sc.take<uint64_t>(nq + 1);
            w.starts = starts;
            scope->summary_slot = 0;
            launch_cross_within(scope, w, false);
            launch_within_offsets(scope, w.counts, nq, (uint32_t)slices, block_sums, starts, offs);
            const uint64_t total = read_total(offs);
            const CallSummary sm = scope->summary_host[0];
            if (!sm.violation) {
                finish_offsets(offs);
                if (total && total <= r.capacity) {
                    stage_outputs(total);
                    w.total = total; w.indices = ind; w.distances = dist;
                    launch_cross_within(scope, w, true);
                    finish_outputs(total);
                }
                SWH_HIP_CHECK(hipStreamSynchronize(stream));
                if (scope->profiling && scope->stamps_used) {
                    collect_timing(scope);
                    // the search is named after its walk, also where a tiny call's scan takes longer: the longer of the two passes
                    swh_timing_t &t = scope->last_timing;
                    t.dominant_ms = 0;
                    for (size_t i = 0; i < scope->stamps_used; ++i) {
                        float ms = 0;
                        if (!strcmp(scope->stamps[i].name, "cross_within")) (void)hipEventElapsedTime(&ms, scope->stamps[i].start, scope->stamps[i].stop);
                        if (ms > t.dominant_ms) t.dominant_ms = ms;
                    }
                    snprintf(t.dominant_name, sizeof t.dominant_name, "cross_within");
                    add_to_totals(scope->totals, scope->last_timing);
                }
                scope->last_timing.cells = sm.cells;
                // the tapes, a count and a start per (row, slice), the row offsets and the hits
                scope->last_timing.bytes = p.pa->total_bytes + p.pb->total_bytes + (nq + nc) * ow + n_counts * 12 + (nq + 1) * 8 +
                                           (total <= r.capacity ? total * 8 : 0);
                return swh_success_k;
            }
            // a string longer than the kernel takes (the memory of a prepared tape changed since it was measured): the general path
            scope->stamps_used = 0;
            scope->last_timing = swh_timing_t{};
        }

        // ---- general path: every block scored twice, once to count and once to fill -------------------------------------------------------
        SearchSweep sweep(scope, engine, p, bound);
        const uint64_t tiles = (nq + kWithinScanTile - 1) / kWithinScanTile;
        const size_t need = pad(sweep.q_step * sweep.c_step * 4) + pad(nq * 4) + pad(nq * 8) + pad(tiles * 8) + (dev_o ? 0 : pad((nq + 1) * 8));
        ensure(scope->topk_scratch, scope->topk_scratch_bytes, need);
        Carver sc{scope->topk_scratch, 0, scope->topk_scratch_bytes};
        uint32_t *matrix = sc.take<uint32_t>(sweep.q_step * sweep.c_step);
        uint32_t *counts = sc.take<uint32_t>(nq);
        uint64_t *cursors = sc.take<uint64_t>(nq), *block_sums = sc.take<uint64_t>(tiles);
        uint64_t *offs = dev_o ? (uint64_t *)r.row_offsets : sc.take<uint64_t>(nq + 1);
        SWH_HIP_CHECK(hipMemsetAsync(counts, 0, nq * 4, stream));
        auto no_rows_begin = [](uint64_t, uint64_t) {};   // (counts and cursors span all queries: nothing to open per block)
        swh_status_t status = sweep.walk(matrix, true, error, no_rows_begin, [&](uint64_t q0, uint64_t rows, uint64_t, uint64_t columns, bool) {
            launch_within_count(scope, matrix, rows, columns, bound, counts + q0);
            sweep.time_own_kernels(1);
        });
        if (status != swh_success_k) return status;
        launch_within_offsets(scope, counts, nq, 1, block_sums, cursors, offs);
        sweep.time_own_kernels(2);
        const uint64_t total = read_total(offs);
        finish_offsets(offs);
        if (total && total <= r.capacity) {
            stage_outputs(total);
            status = sweep.walk(matrix, false, error, no_rows_begin, [&](uint64_t q0, uint64_t rows, uint64_t c0, uint64_t columns, bool) {
                launch_within_fill(scope, matrix, rows, columns, c0, bound, cursors + q0, total, ind, dist);
                sweep.time_own_kernels(1);
            });
            if (status != swh_success_k) return status;
            finish_outputs(total);
        }
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        sweep.close("within");
        return swh_success_k;
    });
}

static swh_status_t within_checks(swh_levenshtein_t e, swh_scope_t s, size_t candidates, uint32_t bound, const size_t *row_offsets,
                                  const uint32_t *indices, const uint32_t *distances, size_t capacity, const char **error) {
    if (!s || !e) return fail(error, swh_invalid_argument_k, "null scope or engine");
    if (((Engine *)e)->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (bound == SWH_UNBOUNDED) return fail(error, swh_invalid_argument_k, "a range search needs a bound: without one it is the dense cross-product");
    if (candidates >= 0xFFFFFFFFull) return fail(error, swh_unsupported_length_k, "2^32 - 1 candidates or more");
    if (!row_offsets) return fail(error, swh_invalid_argument_k, "null row_offsets");
    if (!indices != !distances) return fail(error, swh_invalid_argument_k, "indices and distances must both be given, or neither");
    if (!indices && capacity) return fail(error, swh_invalid_argument_k, "a capacity without arrays: the counting call passes NULL, NULL, 0");
    return swh_success_k;
}

static swh_status_t within_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *q, const swh_tape_u64_t *c, bool utf8, uint32_t bound,
                                 const WithinOutputs &outs, const char **error) {
    if (!q) return fail(error, swh_invalid_argument_k, "null tape");
    const size_t candidates = (c ? c : q)->count;
    swh_status_t status = within_checks(e, s, candidates, bound, outs.row_offsets, outs.indices, outs.distances, outs.capacity, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    // (a search without queries prepares nothing, one without candidates the queries alone: the offsets are still written)
    if ((status = call.prepare(q, c, utf8, q->count != 0, q->count && candidates, error)) != swh_success_k) return status;
    return within_run(call.scope, (Engine *)e, call.pair, bound, outs, error);
}
swh_status_t swh_levenshtein_within_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries, const swh_tape_u64_t *candidates,
                                            uint32_t bound, size_t *row_offsets, uint32_t *indices, uint32_t *distances, size_t capacity,
                                            const char **error) {
    return within_tapes(e, s, queries, candidates, false, bound, WithinOutputs{row_offsets, indices, distances, capacity}, error);
}
swh_status_t swh_levenshtein_utf8_within_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries,
                                                 const swh_tape_u64_t *candidates, uint32_t bound, size_t *row_offsets, uint32_t *indices,
                                                 uint32_t *distances, size_t capacity, const char **error) {
    return within_tapes(e, s, queries, candidates, true, bound, WithinOutputs{row_offsets, indices, distances, capacity}, error);
}
swh_status_t swh_levenshtein_within_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *queries,
                                             const swh_prepared_view_t *candidates, uint32_t bound, size_t *row_offsets, uint32_t *indices,
                                             uint32_t *distances, size_t capacity, const char **error) {
    TwoTapeCall call;
    swh_status_t status = call.views(queries, candidates, true, error);
    if (status != swh_success_k) return status;
    if ((status = within_checks(e, s, call.pair.b_count, bound, row_offsets, indices, distances, capacity, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return within_run(call.scope, (Engine *)e, call.pair, bound, WithinOutputs{row_offsets, indices, distances, capacity}, error);
}

// ---- alignments (align.hip) ----------------------------------------------------------------------------------------------------------
// k_align_sizes measures the batch (stored bytes, symbols, cells, the first pair over SWH_ALIGN_MAX_CELLS) and the stored bytes and slot
// sizes are scanned on the device; one read-back of the measurements decides the errors and the chunks, before any output is written.
// Then per chunk of consecutive pairs the forward pass + walk (k_align), the counts scanned into the offsets, and k_align_emit places
// the ops -- no host round trip between the forward pass and the outputs.
// A chunk holds enough pairs to fill the device -- kAlignFillWaves waves per compute unit, a lane per pair -- and, beyond that, as many
// as keep its stored delta vectors near 128 MiB, where the walk still reads the forward pass's stores from the Infinity Cache. Long
// pairs therefore give up the residency rather than the parallelism (1 K protein pairs of 4 K symbols store 6 GB: one chunk).
// STRINGWARS_AMD_ALIGN_CHUNK_KB=n (test library) sets the byte target and drops the fill minimum, to put many chunks in a small test.
constexpr uint64_t kAlignFillWaves = 8;
static const char *align_chunk_hook() {
    static const char *e = test_hook("STRINGWARS_AMD_ALIGN_CHUNK_KB");
    return e;
}
static uint64_t align_chunk_pairs(const Scope *scope, uint64_t count, uint64_t store_total) {
    const char *hook = align_chunk_hook();
    const uint64_t target = hook ? (uint64_t)atol(hook) << 10 : (uint64_t)128 << 20;
    const uint64_t fill = hook ? 1 : (uint64_t)scope->compute_units * kAlignFillWaves * 64;
    const uint64_t mean = std::max<uint64_t>(1, store_total / std::max<uint64_t>(count, 1));
    uint64_t pairs = std::max<uint64_t>(fill, target / mean);
    // no chunk asks for more than half the device memory that is free
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess && free_bytes)
        pairs = std::min<uint64_t>(pairs, std::max<uint64_t>(1, (uint64_t)(free_bytes / 2) / mean));
    return std::max<uint64_t>(1, std::min<uint64_t>(pairs, count));
}

struct AlignOutputs {
    uint32_t *distances;
    uint64_t *offsets;
    uint8_t *ops;
    size_t capacity;
};

static swh_status_t align_run(Scope *scope, const TapePair &p, uint32_t bound, const AlignOutputs &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t count = p.a_count;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        const bool dev_d = is_device_pointer(r.distances), dev_o = is_device_pointer(r.offsets), dev_ops = is_device_pointer(r.ops);
        if (count == 0) {
            const uint64_t zero = 0;
            if (dev_o) SWH_HIP_CHECK(hipMemcpyAsync(r.offsets, &zero, sizeof zero, hipMemcpyHostToDevice, stream)); else r.offsets[0] = 0;
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            return swh_success_k;
        }
        const bool cp = p.pa->utf8;
        AlignTapes t{};
        t.a = prepared_view(p.pa, cp, p.a_first, count);
        t.b = prepared_view(p.pb, cp, p.b_first, count);
        t.a_off64 = cp ? 1 : p.pa->off64;
        t.b_off64 = cp ? 1 : p.pb->off64;
        t.cp = cp ? 1 : 0;
        t.count = count;

        AlignScratch *sc_entry;
        {
            std::lock_guard<std::mutex> hold(g_align_scratch_lock);
            sc_entry = &g_align_scratch[scope];
        }
        // fixed part: sizes | store_base | slot_base | counts | offsets | distances | scan partials
        const size_t partial_words = align_scan_partials(count);
        const size_t fixed = pad(sizeof(AlignSizes)) + 2 * pad((count + 1) * 8) + pad(count * 4) + (dev_o ? 0 : pad((count + 1) * 8)) +
                             (dev_d ? 0 : pad(count * 4)) + pad(partial_words * 8);
        ensure(sc_entry->buf, sc_entry->bytes, fixed);
        Carver sc{sc_entry->buf, 0, sc_entry->bytes};
        AlignSizes *sizes = sc.take<AlignSizes>(1);
        uint64_t *store_base = sc.take<uint64_t>(count + 1), *slot_base = sc.take<uint64_t>(count + 1);
        uint32_t *counts = sc.take<uint32_t>(count);
        uint64_t *offsets = dev_o ? r.offsets : sc.take<uint64_t>(count + 1);
        uint32_t *distances = dev_d ? r.distances : sc.take<uint32_t>(count);
        uint64_t *partials = sc.take<uint64_t>(partial_words);

        AlignSizes init{};
        init.first_oversize = ~0ull;
        SWH_HIP_CHECK(hipMemcpyAsync(sizes, &init, sizeof init, hipMemcpyHostToDevice, stream));
        launch_align_sizes(scope, t, store_base, slot_base, sizes);
        launch_align_scan(scope, store_base, count, partials);
        launch_align_scan(scope, slot_base, count, partials);
        AlignSizes got{};
        SWH_HIP_CHECK(hipMemcpyAsync(&got, sizes, sizeof got, hipMemcpyDeviceToHost, stream));
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        if (got.first_oversize != ~0ull) {
            const size_t i = (size_t)got.first_oversize;
            const uint64_t la = read_offset(t.a.offsets, t.a_off64, i + 1, true, stream) - read_offset(t.a.offsets, t.a_off64, i, true, stream);
            const uint64_t lb = read_offset(t.b.offsets, t.b_off64, i + 1, true, stream) - read_offset(t.b.offsets, t.b_off64, i, true, stream);
            scope->stamps_used = 0;
            return fail(error, swh_unsupported_length_k, "pair %zu: %llu x %llu symbols exceeds SWH_ALIGN_MAX_CELLS (2^30 cells per pair)", i,
                        (unsigned long long)la, (unsigned long long)lb);
        }
        if (r.capacity < got.symbols) {
            scope->stamps_used = 0;
            return fail(error, swh_invalid_argument_k, "ops_capacity %zu is below the %llu symbols of the two tapes", r.capacity,
                        (unsigned long long)got.symbols);
        }

        // chunks of consecutive pairs; where they start in the storage space is read back (one strided copy) to size the largest
        const uint64_t per_chunk = align_chunk_pairs(scope, count, got.store_total);
        const uint64_t chunks = (count + per_chunk - 1) / per_chunk;
        std::vector<uint64_t> starts(chunks + 1, 0);
        if (chunks > 1) {
            SWH_HIP_CHECK(hipMemcpy2DAsync(starts.data(), 8, store_base, per_chunk * 8, 8, chunks, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
        }
        starts[chunks] = got.store_total;
        uint64_t widest = 0;
        for (uint64_t q = 0; q < chunks; ++q) widest = std::max<uint64_t>(widest, starts[q + 1] - starts[q]);
        // variable part: the op slots (whole batch) | staged ops for host outputs | the widest chunk of stored delta vectors
        const size_t store_bytes = (size_t)widest;
        const size_t need = fixed + pad(got.symbols + 16) + (dev_ops ? 0 : pad(got.symbols + 16)) + pad(store_bytes + 16);
        if (need > sc_entry->bytes) {
            // keep what the fixed part already holds: the measurements and scans live there
            char *grown = nullptr;
            const size_t want = need + need / 4 + (1 << 20);
            SWH_HIP_CHECK(hipMalloc((void **)&grown, want));
            SWH_HIP_CHECK(hipMemcpyAsync(grown, sc_entry->buf, fixed, hipMemcpyDeviceToDevice, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            SWH_HIP_CHECK(hipFree(sc_entry->buf));
            sc_entry->buf = grown;
            sc_entry->bytes = want;
            sc = Carver{grown, 0, want};
            sizes = sc.take<AlignSizes>(1);
            store_base = sc.take<uint64_t>(count + 1); slot_base = sc.take<uint64_t>(count + 1);
            counts = sc.take<uint32_t>(count);
            offsets = dev_o ? r.offsets : sc.take<uint64_t>(count + 1);
            distances = dev_d ? r.distances : sc.take<uint32_t>(count);
            partials = sc.take<uint64_t>(partial_words);
        }
        uint8_t *slots = sc.take<uint8_t>(got.symbols + 16);
        uint8_t *ops = dev_ops ? r.ops : sc.take<uint8_t>(got.symbols + 16);
        char *store = sc.take<char>(store_bytes + 16);

        AlignChunk c{};
        c.store_base = store_base; c.slot_base = slot_base; c.store = store; c.slots = slots;
        c.counts = counts; c.distances = distances; c.bound = bound;
        for (uint64_t q = 0; q < chunks; ++q) {
            c.pair_first = q * per_chunk;
            c.pair_end = std::min<uint64_t>(count, (q + 1) * per_chunk);
            c.store_first = starts[q];
            launch_align_chunk(scope, t, c);
        }
        launch_align_scan_counts(scope, counts, offsets, count, partials);
        launch_align_emit(scope, count, slot_base, counts, offsets, slots, ops);
        if (!dev_d) SWH_HIP_CHECK(hipMemcpyAsync(r.distances, distances, count * 4, hipMemcpyDeviceToHost, stream));
        if (!dev_o) SWH_HIP_CHECK(hipMemcpyAsync(r.offsets, offsets, (count + 1) * 8, hipMemcpyDeviceToHost, stream));
        if (!dev_ops) {
            uint64_t total_ops = 0;
            SWH_HIP_CHECK(hipMemcpyAsync(&total_ops, offsets + count, 8, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            if (total_ops) SWH_HIP_CHECK(hipMemcpyAsync(r.ops, ops, total_ops, hipMemcpyDeviceToHost, stream));
        }
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        if (scope->profiling && scope->stamps_used) {
            collect_timing(scope);
            add_to_totals(scope->totals, scope->last_timing);
        }
        scope->stamps_used = 0;
        scope->last_timing.cells = got.cells;
        scope->last_timing.bytes = (cp ? 4 : 1) * got.symbols + 2 * (count + 1) * 8 + count * 4 + got.symbols;
        return swh_success_k;
    });
}

static swh_status_t align_checks(swh_levenshtein_t e, swh_scope_t s, size_t a_count, size_t b_count, const uint32_t *distances,
                                 const uint64_t *offsets, const uint8_t *ops, const char **error) {
    if (!s || !e) return fail(error, swh_invalid_argument_k, "null scope or engine");
    const Engine *engine = (const Engine *)e;
    if (engine->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (!engine->unit_costs) return fail(error, swh_not_implemented_k, "alignments need unit costs (match 0, mismatch 1, open 1, extend 1)");
    if (a_count != b_count) return fail(error, swh_invalid_argument_k, "a and b must hold the same number of strings");
    if (!offsets || (a_count && (!distances || !ops))) return fail(error, swh_invalid_argument_k, "null output pointer");
    return swh_success_k;
}

static swh_status_t align_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, bool utf8, uint32_t bound,
                                const AlignOutputs &outs, const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    swh_status_t status = align_checks(e, s, a->count, b->count, outs.distances, outs.offsets, outs.ops, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    const bool pairs = a->count != 0;
    if ((status = call.prepare(a, b, utf8, pairs, pairs, error)) != swh_success_k) return status;
    return align_run(call.scope, call.pair, bound, outs, error);
}
swh_status_t swh_levenshtein_align_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, uint32_t bound,
                                           uint32_t *distances, size_t *ops_offsets, char *ops, size_t ops_capacity, const char **error) {
    return align_tapes(e, s, a, b, false, bound, AlignOutputs{distances, (uint64_t *)ops_offsets, (uint8_t *)ops, ops_capacity}, error);
}
swh_status_t swh_levenshtein_utf8_align_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                uint32_t bound, uint32_t *distances, size_t *ops_offsets, char *ops, size_t ops_capacity,
                                                const char **error) {
    return align_tapes(e, s, a, b, true, bound, AlignOutputs{distances, (uint64_t *)ops_offsets, (uint8_t *)ops, ops_capacity}, error);
}
swh_status_t swh_levenshtein_align_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                            uint32_t bound, uint32_t *distances, size_t *ops_offsets, char *ops, size_t ops_capacity,
                                            const char **error) {
    const AlignOutputs outs{distances, (uint64_t *)ops_offsets, (uint8_t *)ops, ops_capacity};
    TwoTapeCall call;
    swh_status_t status = call.views(a, b, false, error);
    if (status != swh_success_k) return status;
    if ((status = align_checks(e, s, call.pair.a_count, call.pair.b_count, outs.distances, outs.offsets, outs.ops, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return align_run(call.scope, call.pair, bound, outs, error);
}

// ---- infix search (infix.hip) ---------------------------------------------------------------------------------------------------------
// k_infix_sizes measures the batch (cells, the first pattern over SWH_INFIX_MAX_PATTERN) and cuts it into work items; one read-back of
// the measurements decides the errors before any output is written. Then the forward pass (distance and end of every pair) and the
// start pass (the starts, the bound) over the same items, and the copy-out of outputs that live on the host. The scratch -- the item
// list and, for host outputs, the three result arrays -- is the scope's alignment scratch: both calls are synchronous.
struct InfixOutputs { uint32_t *distances, *starts, *ends; };

static swh_status_t infix_run(Scope *scope, const TapePair &p, uint32_t bound, const InfixOutputs &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t count = p.a_count;
        if (count == 0) return swh_success_k;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        const bool dev_d = is_device_pointer(r.distances), dev_s = is_device_pointer(r.starts), dev_e = is_device_pointer(r.ends);
        const bool cp = p.pa->utf8;
        InfixTapes t{};
        t.patterns = prepared_view(p.pa, cp, p.a_first, count);
        t.texts = prepared_view(p.pb, cp, p.b_first, count);
        t.p_off64 = cp ? 1 : p.pa->off64;
        t.t_off64 = cp ? 1 : p.pb->off64;
        t.cp = cp ? 1 : 0;
        t.count = count;

        AlignScratch *sc_entry;
        {
            std::lock_guard<std::mutex> hold(g_align_scratch_lock);
            sc_entry = &g_align_scratch[scope];
        }
        // sizes | items | distances | starts | ends (the last three only where the caller's array lives on the host)
        const size_t need = pad(sizeof(InfixSizes)) + pad(count * sizeof(LaneItem)) + ((dev_d ? 0 : 1) + (dev_s ? 0 : 1) + (dev_e ? 0 : 1)) * pad(count * 4);
        ensure(sc_entry->buf, sc_entry->bytes, need);
        Carver sc{sc_entry->buf, 0, sc_entry->bytes};
        InfixSizes *sizes = sc.take<InfixSizes>(1);
        LaneItem *items = sc.take<LaneItem>(count);
        uint32_t *distances = dev_d ? r.distances : sc.take<uint32_t>(count);
        uint32_t *starts = dev_s ? r.starts : sc.take<uint32_t>(count);
        uint32_t *ends = dev_e ? r.ends : sc.take<uint32_t>(count);

        InfixSizes init{};
        init.first_oversize = ~0ull;
        SWH_HIP_CHECK(hipMemcpyAsync(sizes, &init, sizeof init, hipMemcpyHostToDevice, stream));
        launch_infix_sizes(scope, t, sizes, items);
        InfixSizes got{};
        SWH_HIP_CHECK(hipMemcpyAsync(&got, sizes, sizeof got, hipMemcpyDeviceToHost, stream));
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        if (got.first_oversize != ~0ull) {
            const size_t i = (size_t)got.first_oversize;
            const uint64_t m = read_offset(t.patterns.offsets, t.p_off64, i + 1, true, stream) - read_offset(t.patterns.offsets, t.p_off64, i, true, stream);
            scope->stamps_used = 0;
            return fail(error, swh_unsupported_length_k, "pair %zu: a pattern of %llu symbols exceeds SWH_INFIX_MAX_PATTERN (2048)", i,
                        (unsigned long long)m);
        }

        InfixRun run{};
        run.items = items; run.item_count = got.items;
        run.distances = distances; run.starts = starts; run.ends = ends;
        run.bound = bound;
        run.wide_text = !cp && got.text_symbols >= 16;
        launch_infix_forward(scope, t, run);
        launch_infix_starts(scope, t, run);
        if (!dev_d) SWH_HIP_CHECK(hipMemcpyAsync(r.distances, distances, count * 4, hipMemcpyDeviceToHost, stream));
        if (!dev_s) SWH_HIP_CHECK(hipMemcpyAsync(r.starts, starts, count * 4, hipMemcpyDeviceToHost, stream));
        if (!dev_e) SWH_HIP_CHECK(hipMemcpyAsync(r.ends, ends, count * 4, hipMemcpyDeviceToHost, stream));
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        if (scope->profiling && scope->stamps_used) {
            collect_timing(scope);
            add_to_totals(scope->totals, scope->last_timing);
        }
        scope->stamps_used = 0;
        scope->last_timing.cells = got.cells;
        scope->last_timing.bytes = (cp ? 4 : 1) * got.symbols + 2 * (count + 1) * 8 + 3 * count * 4;
        return swh_success_k;
    });
}

// no scope or engine can exist without a device: a call that gets a null handle says so where there is none, as scope creation does
// (infix search and the scored families ask; top-k, within and align answer "null scope or engine" without the probe)
static swh_status_t probe_null_handles(swh_levenshtein_t e, swh_scope_t s, const char **error) {
    if (s && e) return swh_success_k;
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) {
        (void)hipGetLastError();
        return fail(error, swh_no_device_k, "no HIP device visible (this backend has no CPU path)");
    }
    return fail(error, swh_invalid_argument_k, "null scope or engine");
}
static swh_status_t infix_checks(swh_levenshtein_t e, swh_scope_t s, size_t p_count, size_t t_count, const uint32_t *distances,
                                 const uint32_t *starts, const uint32_t *ends, const char **error) {
    const Engine *engine = (const Engine *)e;
    if (engine->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (!engine->unit_costs) return fail(error, swh_not_implemented_k, "infix search needs unit costs (match 0, mismatch 1, open 1, extend 1)");
    if (p_count != t_count) return fail(error, swh_invalid_argument_k, "patterns and texts must hold the same number of strings");
    if (p_count && (!distances || !starts || !ends)) return fail(error, swh_invalid_argument_k, "null output pointer");
    return swh_success_k;
}

static swh_status_t infix_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *patterns, const swh_tape_u64_t *texts, bool utf8,
                                uint32_t bound, const InfixOutputs &outs, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (!patterns || !texts) return fail(error, swh_invalid_argument_k, "null tape");
    status = infix_checks(e, s, patterns->count, texts->count, outs.distances, outs.starts, outs.ends, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    const bool pairs = patterns->count != 0;
    if ((status = call.prepare(patterns, texts, utf8, pairs, pairs, error)) != swh_success_k) return status;
    return infix_run(call.scope, call.pair, bound, outs, error);
}
swh_status_t swh_levenshtein_infix_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *patterns, const swh_tape_u64_t *texts,
                                           uint32_t bound, uint32_t *distances, uint32_t *starts, uint32_t *ends, const char **error) {
    return infix_tapes(e, s, patterns, texts, false, bound, InfixOutputs{distances, starts, ends}, error);
}
swh_status_t swh_levenshtein_utf8_infix_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *patterns, const swh_tape_u64_t *texts,
                                                uint32_t bound, uint32_t *distances, uint32_t *starts, uint32_t *ends, const char **error) {
    return infix_tapes(e, s, patterns, texts, true, bound, InfixOutputs{distances, starts, ends}, error);
}
swh_status_t swh_levenshtein_infix_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *patterns,
                                            const swh_prepared_view_t *texts, uint32_t bound, uint32_t *distances, uint32_t *starts,
                                            uint32_t *ends, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.views(patterns, texts, false, error)) != swh_success_k) return status;
    if ((status = infix_checks(e, s, call.pair.a_count, call.pair.b_count, distances, starts, ends, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return infix_run(call.scope, call.pair, bound, InfixOutputs{distances, starts, ends}, error);
}

// ---- OSA distances, LCS lengths / Indel distances, Jaro counts (osa.hip, lcs.hip, jaro.hip): one planner --------------------------------
// The three families score pairs on the same phases. A sizes kernel measures the pairs (cells, symbols, the first pair over the
// family's length limit) and cuts them into work items; one read-back of the measurements decides the errors before any output is
// written; the family's kernel scores the items and writes whichever of its outputs the caller asked for. A pairwise call is one such
// round. A cross-product maps pair p to (p / nb, p % nb) and runs in slices of whole rows of about kScoredChunkPairs pairs -- the item
// list and, per output that lives on the host, the staged slice are all the scratch there is, whatever the matrix size; with more
// than one slice the whole matrix is measured first (no items), so that a refusal still comes before the first row is written. The
// family's test hook (test library) lowers the slice, to put many of them in a small test. The scratch is the scope's alignment
// scratch: the calls are synchronous, and they learn nothing into the scope.
// What a family brings is its ScoredFamily: the two launchers, its words, and the few argument rules that differ.
//  - OSA: k_osa_sizes cuts the items by the blocks of a pair's shorter string, which holds at most SWH_OSA_MAX_SHORTER symbols; one output.
//  - LCS / Indel: OSA's sizes kernel and limit as they stand (SWH_LCS_MAX_SHORTER); two outputs, indel and lcs.
//  - Jaro: k_jaro_sizes cuts the items by the blocks of b, and neither string holds more than SWH_JARO_MAX_LENGTH symbols; three
//    outputs, matches, transpositions and prefix, and the only family that holds strides to multiples of the element.
constexpr uint64_t kScoredChunkPairs = (uint64_t)1 << 21;
constexpr int kScoredOutputs = 3;

struct ScoredFamily {
    int outputs;   // of kScoredOutputs
    void (*sizes)(Scope *scope, const OsaTapes &t, OsaSizes *sizes, LaneItem *items);
    // scores the items into where[0 .. outputs), null where an output is not written by this launch, all at `stride`
    void (*launch)(Scope *scope, const OsaTapes &t, const LaneItem *items, uint64_t item_count, char *const where[kScoredOutputs], uint64_t stride,
                   uint32_t bound, bool wide);
    const char *chunk_hook;      // the test hook that lowers the slice
    const char *oversize;        // how the refusal of a pair over the length limit ends
    const char *unit_costs;      // the refusal of a general-cost engine
    const char *null_outputs;    // the refusal of a call that wants no output ...
    bool null_outputs_on_empty;  // ... which a call without pairs meets too
    bool element_strides;        // strides are multiples of the element (4 bytes pairwise, 8 cross), not merely large enough
};

static const ScoredFamily kOsaFamily = {
    1, launch_osa_sizes,
    [](Scope *scope, const OsaTapes &t, const LaneItem *items, uint64_t item_count, char *const where[kScoredOutputs], uint64_t stride, uint32_t bound,
       bool wide) {
        OsaRun run{};
        run.items = items; run.item_count = item_count;
        run.out = where[0];
        run.stride = stride; run.bound = bound; run.wide = wide;
        launch_osa(scope, t, run);
    },
    "STRINGWARS_AMD_OSA_CHUNK_PAIRS", "the shorter string exceeds SWH_OSA_MAX_SHORTER (2048)",
    "OSA distances need unit costs (match 0, mismatch 1, open 1, extend 1)", "null output pointer", false, false};
static const ScoredFamily kLcsFamily = {
    2, launch_osa_sizes,
    [](Scope *scope, const OsaTapes &t, const LaneItem *items, uint64_t item_count, char *const where[kScoredOutputs], uint64_t stride, uint32_t bound,
       bool wide) {
        LcsRun run{};
        run.items = items; run.item_count = item_count;
        run.indel = where[0]; run.lcs = where[1];
        run.stride = stride; run.bound = bound; run.wide = wide;
        launch_lcs(scope, t, run);
    },
    "STRINGWARS_AMD_LCS_CHUNK_PAIRS", "the shorter string exceeds SWH_LCS_MAX_SHORTER (2048)",
    "LCS lengths and Indel distances are called on a unit-cost engine (match 0, mismatch 1, open 1, extend 1)",
    "null output pointers: one of indel and lcs is needed", true, false};
static const ScoredFamily kJaroFamily = {
    3, launch_jaro_sizes,
    [](Scope *scope, const OsaTapes &t, const LaneItem *items, uint64_t item_count, char *const where[kScoredOutputs], uint64_t stride, uint32_t,
       bool wide) {
        JaroRun run{};
        run.items = items; run.item_count = item_count;
        run.matches = where[0]; run.transpositions = where[1]; run.prefix = where[2];
        run.stride = stride; run.wide = wide;
        launch_jaro(scope, t, run);
    },
    "STRINGWARS_AMD_JARO_CHUNK_PAIRS", "a string exceeds SWH_JARO_MAX_LENGTH (2048)",
    "Jaro and Jaro-Winkler counts are called on a unit-cost engine (match 0, mismatch 1, open 1, extend 1)",
    "null output pointers: one of matches, transpositions and prefix is needed", true, true};

static uint64_t scored_chunk_pairs(const ScoredFamily &f) {
    const char *hook = test_hook(f.chunk_hook);
    const uint64_t pairs = hook ? (uint64_t)atoll(hook) : kScoredChunkPairs;
    return std::max<uint64_t>(1, std::min<uint64_t>(pairs, kScoredChunkPairs));
}

struct ScoredRequest {
    bool cross;
    uint32_t bound;
    void *outs[kScoredOutputs];   // the family's outputs in the order of its exports: any may be null, those past its count are
    size_t stride;                // bytes between consecutive results (pairs) or rows (cross), of every output
};

static swh_status_t scored_run(Scope *scope, const ScoredFamily &f, const TapePair &p, const ScoredRequest &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t na = p.a_count, nb = p.b_count;
        if (na == 0 || nb == 0) return swh_success_k;
        if (r.cross && na > ((uint64_t)1 << 40) / nb) return fail(error, swh_unsupported_length_k, "more than 2^40 pairs in one call");
        const uint64_t total = r.cross ? na * nb : na;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        bool stage[kScoredOutputs];
        size_t staged_count = 0, wanted = 0;
        for (int k = 0; k < f.outputs; ++k) {
            stage[k] = r.outs[k] && !is_device_pointer(r.outs[k]);
            staged_count += stage[k] ? 1 : 0;
            wanted += r.outs[k] ? 1 : 0;
        }
        const bool cp = p.pa->utf8;
        OsaTapes t{};
        t.a = prepared_view(p.pa, cp, p.a_first, na);
        t.b = prepared_view(p.pb, cp, p.b_first, nb);
        t.a_off64 = cp ? 1 : p.pa->off64;
        t.b_off64 = cp ? 1 : p.pb->off64;
        t.cp = cp ? 1 : 0;
        t.nb = r.cross ? nb : 0;

        // slices: all pairs of a pairwise call; whole rows of a cross-product
        const uint64_t rows_per_slice = r.cross ? std::max<uint64_t>(1, scored_chunk_pairs(f) / nb) : na;
        const uint64_t slices = (na + rows_per_slice - 1) / rows_per_slice;
        const uint64_t slice_pairs = r.cross ? std::min<uint64_t>(rows_per_slice, na) * nb : na;
        const size_t width = r.cross ? 8 : 4;

        AlignScratch *sc_entry;
        {
            std::lock_guard<std::mutex> hold(g_align_scratch_lock);
            sc_entry = &g_align_scratch[scope];
        }
        // sizes | items | the slice's results (one array per output that lives on the host)
        const size_t need = pad(sizeof(OsaSizes)) + pad(slice_pairs * sizeof(LaneItem)) + staged_count * pad(slice_pairs * width);
        ensure(sc_entry->buf, sc_entry->bytes, need);
        Carver sc{sc_entry->buf, 0, sc_entry->bytes};
        OsaSizes *sizes = sc.take<OsaSizes>(1);
        LaneItem *items = sc.take<LaneItem>(slice_pairs);
        char *staged[kScoredOutputs];
        for (int k = 0; k < f.outputs; ++k) staged[k] = stage[k] ? sc.take<char>(slice_pairs * width) : nullptr;

        // measures pairs [row0 .. row0 + rows) x nb (or all pairs of a pairwise call) and, with `cut`, cuts them into `items`
        auto measure = [&](uint64_t row0, uint64_t pairs, bool cut) {
            OsaSizes init{};
            init.first_oversize = ~0ull;
            SWH_HIP_CHECK(hipMemcpyAsync(sizes, &init, sizeof init, hipMemcpyHostToDevice, stream));
            t.row0 = row0; t.count = pairs;
            f.sizes(scope, t, sizes, cut ? items : nullptr);
            OsaSizes got{};
            SWH_HIP_CHECK(hipMemcpyAsync(&got, sizes, sizeof got, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            return got;
        };
        const OsaSizes whole = measure(0, total, slices == 1);
        if (whole.first_oversize != ~0ull) {
            const size_t i = (size_t)(r.cross ? whole.first_oversize / nb : whole.first_oversize);
            const size_t j = (size_t)(r.cross ? whole.first_oversize % nb : whole.first_oversize);
            const uint64_t la = read_offset(t.a.offsets, t.a_off64, i + 1, true, stream) - read_offset(t.a.offsets, t.a_off64, i, true, stream);
            const uint64_t lb = read_offset(t.b.offsets, t.b_off64, j + 1, true, stream) - read_offset(t.b.offsets, t.b_off64, j, true, stream);
            scope->stamps_used = 0;
            if (r.cross)
                return fail(error, swh_unsupported_length_k, "pair (%zu, %zu): %llu x %llu symbols, %s", i, j, (unsigned long long)la,
                            (unsigned long long)lb, f.oversize);
            return fail(error, swh_unsupported_length_k, "pair %zu: %llu x %llu symbols, %s", i, (unsigned long long)la, (unsigned long long)lb,
                        f.oversize);
        }

        const bool wide = !cp && whole.a_total >= 16 && whole.b_total >= 16;
        // the kernel writes its outputs at one stride: the caller's for those written in place, the packed one for those that are
        // staged; a call with outputs of both kinds runs the slice once per kind
        for (uint64_t q = 0; q < slices; ++q) {
            const uint64_t row0 = q * rows_per_slice, rows = std::min<uint64_t>(rows_per_slice, na - row0);
            const uint64_t pairs = r.cross ? rows * nb : na;
            const uint64_t item_count = slices == 1 ? whole.items : measure(row0, pairs, true).items;
            t.row0 = row0; t.count = pairs;
            for (int packed = 0; packed < 2; ++packed) {
                char *where[kScoredOutputs] = {};
                bool any = false;
                for (int k = 0; k < f.outputs; ++k) {
                    if (!r.outs[k] || stage[k] != (packed == 1)) continue;
                    where[k] = packed ? staged[k] : (char *)r.outs[k] + (r.cross ? row0 * r.stride : 0);
                    any = true;
                }
                if (any) f.launch(scope, t, items, item_count, where, packed ? (r.cross ? nb * 8 : 4) : r.stride, r.bound, wide);
            }
            for (int k = 0; k < f.outputs; ++k) {
                if (!stage[k]) continue;
                if (r.cross)
                    SWH_HIP_CHECK(hipMemcpy2DAsync((char *)r.outs[k] + row0 * r.stride, r.stride, staged[k], nb * 8, nb * 8, rows, hipMemcpyDeviceToHost, stream));
                else if (r.stride == 4)
                    SWH_HIP_CHECK(hipMemcpyAsync(r.outs[k], staged[k], pairs * 4, hipMemcpyDeviceToHost, stream));
                else
                    SWH_HIP_CHECK(hipMemcpy2DAsync(r.outs[k], r.stride, staged[k], 4, 4, pairs, hipMemcpyDeviceToHost, stream));
            }
            if (staged_count) SWH_HIP_CHECK(hipStreamSynchronize(stream));   // the next slice reuses the staging
        }
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        if (scope->profiling && scope->stamps_used) {
            collect_timing(scope);
            add_to_totals(scope->totals, scope->last_timing);
        }
        scope->stamps_used = 0;
        scope->last_timing.cells = whole.cells;
        scope->last_timing.bytes = (cp ? 4 : 1) * whole.symbols + (na + nb + 2) * 8 + total * width * wanted;
        return swh_success_k;
    });
}

// the argument rules; a stride of 0 becomes the packed one
static swh_status_t scored_checks(const ScoredFamily &f, swh_levenshtein_t e, size_t a_count, size_t b_count, bool cross,
                                  void *const (&outs)[kScoredOutputs], size_t &stride, const char **error) {
    const Engine *engine = (const Engine *)e;
    if (engine->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (!engine->unit_costs) return fail(error, swh_not_implemented_k, "%s", f.unit_costs);
    if (!cross && a_count != b_count) return fail(error, swh_invalid_argument_k, "a and b must hold the same number of strings");
    bool wanted = false;
    for (int k = 0; k < f.outputs; ++k) wanted = wanted || outs[k];
    if (!wanted && (f.null_outputs_on_empty || (a_count && b_count))) return fail(error, swh_invalid_argument_k, "%s", f.null_outputs);
    if (cross) {
        if (!stride) stride = b_count * 8;
        if (f.element_strides && stride % 8) return fail(error, swh_invalid_argument_k, "row_stride_bytes must be 0 or a multiple of 8");
        if (stride < b_count * 8) return fail(error, swh_invalid_argument_k, "row_stride_bytes too small");
    } else {
        if (!stride) stride = 4;
        if (f.element_strides && stride % 4) return fail(error, swh_invalid_argument_k, "out_stride_bytes must be 0 or a multiple of 4");
        if (stride < 4) return fail(error, swh_invalid_argument_k, "out_stride_bytes must be >= 4");
    }
    return swh_success_k;
}

static swh_status_t scored_tapes(const ScoredFamily &f, swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                 bool utf8, bool cross, uint32_t bound, void *const (&outs)[kScoredOutputs], size_t stride, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (!a || (!b && !cross)) return fail(error, swh_invalid_argument_k, "null tape");
    const size_t b_count = (b ? b : a)->count;   // a cross-product without b: the self-product
    status = scored_checks(f, e, a->count, b_count, cross, outs, stride, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    const bool pairs = a->count && b_count;
    if ((status = call.prepare(a, b, utf8, pairs, pairs, error)) != swh_success_k) return status;
    return scored_run(call.scope, f, call.pair, ScoredRequest{cross, bound, {outs[0], outs[1], outs[2]}, stride}, error);
}
static swh_status_t scored_prepared(const ScoredFamily &f, swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a,
                                    const swh_prepared_view_t *b, bool cross, uint32_t bound, void *const (&outs)[kScoredOutputs], size_t stride,
                                    const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.views(a, b, cross, error)) != swh_success_k) return status;
    if ((status = scored_checks(f, e, call.pair.a_count, call.pair.b_count, cross, outs, stride, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return scored_run(call.scope, f, call.pair, ScoredRequest{cross, bound, {outs[0], outs[1], outs[2]}, stride}, error);
}

swh_status_t swh_levenshtein_osa_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, uint32_t bound,
                                               uint32_t *out, size_t stride, const char **error) {
    return scored_tapes(kOsaFamily, e, s, a, b, false, false, bound, {out}, stride, error);
}
swh_status_t swh_levenshtein_utf8_osa_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                    uint32_t bound, uint32_t *out, size_t stride, const char **error) {
    return scored_tapes(kOsaFamily, e, s, a, b, true, false, bound, {out}, stride, error);
}
swh_status_t swh_levenshtein_osa_pairs_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                uint32_t bound, uint32_t *out, size_t stride, const char **error) {
    return scored_prepared(kOsaFamily, e, s, a, b, false, bound, {out}, stride, error);
}
swh_status_t swh_levenshtein_osa_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, size_t *out,
                                               size_t row_stride, const char **error) {
    return scored_tapes(kOsaFamily, e, s, a, b, false, true, SWH_UNBOUNDED, {out}, row_stride, error);
}
swh_status_t swh_levenshtein_utf8_osa_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                    size_t *out, size_t row_stride, const char **error) {
    return scored_tapes(kOsaFamily, e, s, a, b, true, true, SWH_UNBOUNDED, {out}, row_stride, error);
}
swh_status_t swh_levenshtein_osa_cross_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                size_t *out, size_t row_stride, const char **error) {
    return scored_prepared(kOsaFamily, e, s, a, b, true, SWH_UNBOUNDED, {out}, row_stride, error);
}

swh_status_t swh_levenshtein_lcs_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, uint32_t bound,
                                               uint32_t *indel, uint32_t *lcs, size_t stride, const char **error) {
    return scored_tapes(kLcsFamily, e, s, a, b, false, false, bound, {indel, lcs}, stride, error);
}
swh_status_t swh_levenshtein_utf8_lcs_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                    uint32_t bound, uint32_t *indel, uint32_t *lcs, size_t stride, const char **error) {
    return scored_tapes(kLcsFamily, e, s, a, b, true, false, bound, {indel, lcs}, stride, error);
}
swh_status_t swh_levenshtein_lcs_pairs_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                uint32_t bound, uint32_t *indel, uint32_t *lcs, size_t stride, const char **error) {
    return scored_prepared(kLcsFamily, e, s, a, b, false, bound, {indel, lcs}, stride, error);
}
swh_status_t swh_levenshtein_lcs_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, size_t *indel,
                                               size_t *lcs, size_t row_stride, const char **error) {
    return scored_tapes(kLcsFamily, e, s, a, b, false, true, SWH_UNBOUNDED, {indel, lcs}, row_stride, error);
}
swh_status_t swh_levenshtein_utf8_lcs_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                    size_t *indel, size_t *lcs, size_t row_stride, const char **error) {
    return scored_tapes(kLcsFamily, e, s, a, b, true, true, SWH_UNBOUNDED, {indel, lcs}, row_stride, error);
}
swh_status_t swh_levenshtein_lcs_cross_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                size_t *indel, size_t *lcs, size_t row_stride, const char **error) {
    return scored_prepared(kLcsFamily, e, s, a, b, true, SWH_UNBOUNDED, {indel, lcs}, row_stride, error);
}

// (the Jaro kernel takes no bound)
swh_status_t swh_levenshtein_jaro_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                uint32_t *matches, uint32_t *transpositions, uint32_t *prefix, size_t stride, const char **error) {
    return scored_tapes(kJaroFamily, e, s, a, b, false, false, SWH_UNBOUNDED, {matches, transpositions, prefix}, stride, error);
}
swh_status_t swh_levenshtein_utf8_jaro_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                     uint32_t *matches, uint32_t *transpositions, uint32_t *prefix, size_t stride, const char **error) {
    return scored_tapes(kJaroFamily, e, s, a, b, true, false, SWH_UNBOUNDED, {matches, transpositions, prefix}, stride, error);
}
swh_status_t swh_levenshtein_jaro_pairs_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                 uint32_t *matches, uint32_t *transpositions, uint32_t *prefix, size_t stride, const char **error) {
    return scored_prepared(kJaroFamily, e, s, a, b, false, SWH_UNBOUNDED, {matches, transpositions, prefix}, stride, error);
}
swh_status_t swh_levenshtein_jaro_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                size_t *matches, size_t *transpositions, size_t *prefix, size_t row_stride, const char **error) {
    return scored_tapes(kJaroFamily, e, s, a, b, false, true, SWH_UNBOUNDED, {matches, transpositions, prefix}, row_stride, error);
}
swh_status_t swh_levenshtein_utf8_jaro_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                     size_t *matches, size_t *transpositions, size_t *prefix, size_t row_stride, const char **error) {
    return scored_tapes(kJaroFamily, e, s, a, b, true, true, SWH_UNBOUNDED, {matches, transpositions, prefix}, row_stride, error);
}
swh_status_t swh_levenshtein_jaro_cross_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                 size_t *matches, size_t *transpositions, size_t *prefix, size_t row_stride, const char **error) {
    return scored_prepared(kJaroFamily, e, s, a, b, true, SWH_UNBOUNDED, {matches, transpositions, prefix}, row_stride, error);
}

// ---- score search (extract.hip): the k best candidates by an OSA, Indel, LCS, ratio, Jaro or Jaro-Winkler score ------------------------
// topk_run's general path with the three families as the scorers: query blocks x candidate slices of at most kScoredChunkPairs
// pairs, each slice measured and cut into items by the family's sizes kernel, scored by its launcher into dense u64 counts in scratch
// (the candidates' slice is a view of the prepared tape: pair p of the launch is (p / columns, p % columns)) and folded into the
// block's running lists by k_extract_select, which evaluates the float64 score. The scratch is the slice's items and counts, the
// block's lists and, for outputs in host memory, the rows: nothing grows with queries x candidates. Both length limits follow from
// the two tapes' own lengths, so one pass over their offsets refuses the call before anything is scored or written.
// STRINGWARS_AMD_EXTRACT_CHUNK_PAIRS (test library) lowers the slice, to put several blocks and slices into a small test.
static uint64_t extract_chunk_pairs() {
    const char *hook = test_hook("STRINGWARS_AMD_EXTRACT_CHUNK_PAIRS");
    const uint64_t pairs = hook ? (uint64_t)atoll(hook) : kScoredChunkPairs;
    return std::max<uint64_t>(1, std::min<uint64_t>(pairs, kScoredChunkPairs));
}

struct ExtractRequest {
    int scorer;
    uint32_t k;
    double cutoff, prefix_weight;
    uint32_t *indices;
    void *scores;
};

static swh_status_t extract_run(Scope *scope, const TapePair &p, const ExtractRequest &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t nq = p.a_count, nc = p.b_count, k = r.k;
        if (nq == 0) return swh_success_k;
        const size_t index_bytes = nq * k * sizeof(uint32_t), score_bytes = nq * k * sizeof(uint64_t);
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        const bool dev_i = is_device_pointer(r.indices), dev_s = is_device_pointer(r.scores);
        if (nc == 0) {   // every row is padding
            if (dev_i) SWH_HIP_CHECK(hipMemsetAsync(r.indices, 0xFF, index_bytes, stream)); else memset(r.indices, 0xFF, index_bytes);
            if (dev_s) SWH_HIP_CHECK(hipMemsetAsync(r.scores, 0xFF, score_bytes, stream)); else memset(r.scores, 0xFF, score_bytes);
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            return swh_success_k;
        }
        const bool jaro = r.scorer >= SWH_SCORER_JARO;
        const ScoredFamily &f = r.scorer == SWH_SCORER_OSA ? kOsaFamily : (jaro ? kJaroFamily : kLcsFamily);
        const int counts = r.scorer == SWH_SCORER_JARO_WINKLER ? 3 : (jaro ? 2 : 1);
        const bool cp = p.pa->utf8;
        const uint32_t a_off64 = cp ? 1 : p.pa->off64, b_off64 = cp ? 1 : p.pb->off64;
        const TapeRef queries = prepared_view(p.pa, cp, p.a_first, nq), candidates = prepared_view(p.pb, cp, p.b_first, nc);

        // query blocks of at most 4096 rows x candidate slices, at least 64 columns wide where the slice allows it
        const uint64_t chunk = extract_chunk_pairs();
        const uint64_t q_step = std::min<uint64_t>(nq, std::max<uint64_t>(1, std::min<uint64_t>(4096, chunk >> 6)));
        const uint64_t c_step = std::max<uint64_t>(1, std::min<uint64_t>(nc, chunk / q_step));
        const uint64_t slice_pairs = q_step * c_step;

        // first over-long strings | sizes | items | the slice's counts | the block's lists | rows bound for the host
        const size_t need = pad(2 * sizeof(unsigned long long)) + pad(sizeof(OsaSizes)) + pad(slice_pairs * sizeof(LaneItem)) +
                            counts * pad(slice_pairs * 8) + pad(q_step * k * 16) + (dev_i ? 0 : pad(index_bytes)) + (dev_s ? 0 : pad(score_bytes));
        ensure(scope->topk_scratch, scope->topk_scratch_bytes, need);
        Carver sc{scope->topk_scratch, 0, scope->topk_scratch_bytes};
        unsigned long long *first_over = sc.take<unsigned long long>(2);
        OsaSizes *sizes = sc.take<OsaSizes>(1);
        LaneItem *items = sc.take<LaneItem>(slice_pairs);
        uint64_t *slice[kScoredOutputs] = {};
        for (int o = 0; o < counts; ++o) slice[o] = sc.take<uint64_t>(slice_pairs);
        char *lists = sc.take<char>(q_step * k * 16);
        uint32_t *ind = dev_i ? r.indices : sc.take<uint32_t>(nq * k);
        uint64_t *sco = dev_s ? (uint64_t *)r.scores : sc.take<uint64_t>(nq * k);

        // the search as one call: with profiling on, the kernels since the last absorb() go into the sum (`scoring`: the family's kernel)
        swh_timing_t sum{};
        char scoring_name[40] = "";
        auto absorb = [&](bool scoring) {
            if (scope->profiling && scope->stamps_used) {
                SWH_HIP_CHECK(hipStreamSynchronize(stream));
                collect_timing(scope);
                const swh_timing_t &t = scope->last_timing;
                sum.total_ms += t.total_ms; sum.compute_ms += t.compute_ms; sum.kernels += t.kernels;
                if (scoring) { sum.dominant_ms += t.dominant_ms; snprintf(scoring_name, sizeof scoring_name, "%s", t.dominant_name); }
            }
            scope->stamps_used = 0;
        };

        // the length limits: OSA and LCS refuse a pair whose SHORTER string is over theirs, Jaro one with either string over its own
        SWH_HIP_CHECK(hipMemsetAsync(first_over, 0xFF, 2 * sizeof(unsigned long long), stream));
        const uint32_t limit = jaro ? SWH_JARO_MAX_LENGTH : SWH_OSA_MAX_SHORTER;
        launch_extract_first_over(scope, queries, a_off64, limit, first_over);
        launch_extract_first_over(scope, candidates, b_off64, limit, first_over + 1);
        unsigned long long over[2];
        SWH_HIP_CHECK(hipMemcpyAsync(over, first_over, sizeof over, hipMemcpyDeviceToHost, stream));
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        absorb(false);
        const bool a_over = over[0] != ~0ull, b_over = over[1] != ~0ull;
        if (jaro ? (a_over || b_over) : (a_over && b_over)) {
            const size_t i = a_over ? (size_t)over[0] : 0, j = b_over ? (size_t)over[1] : 0;
            const uint64_t la = read_offset(queries.offsets, a_off64, i + 1, true, stream) - read_offset(queries.offsets, a_off64, i, true, stream);
            const uint64_t lb = read_offset(candidates.offsets, b_off64, j + 1, true, stream) - read_offset(candidates.offsets, b_off64, j, true, stream);
            return fail(error, swh_unsupported_length_k, "pair (%zu, %zu): %llu x %llu symbols, %s", i, j, (unsigned long long)la,
                        (unsigned long long)lb, f.oversize);
        }

        // a finite cutoff of the OSA scorer is the scoring kernel's bound: what it clamps is over the cutoff anyway (the LCS kernel
        // runs unbounded: every scorer of its family reads the LCS length)
        const uint32_t bound = r.scorer == SWH_SCORER_OSA && r.cutoff < 4294967294.0 ? (uint32_t)r.cutoff : SWH_UNBOUNDED;
        uint64_t cutoff_bits;
        memcpy(&cutoff_bits, &r.cutoff, sizeof cutoff_bits);
        uint64_t symbols = 0;
        for (uint64_t q0 = 0; q0 < nq; q0 += q_step) {
            const uint64_t rows = std::min<uint64_t>(q_step, nq - q0);
            SWH_HIP_CHECK(hipMemsetAsync(lists, 0xFF, rows * k * 16, stream));   // every row is padding
            for (uint64_t c0 = 0; c0 < nc; c0 += c_step) {
                const uint64_t columns = std::min<uint64_t>(c_step, nc - c0);
                OsaTapes t{};
                t.a = prepared_view(p.pa, cp, p.a_first + q0, rows);
                t.b = prepared_view(p.pb, cp, p.b_first + c0, columns);
                t.a_off64 = a_off64; t.b_off64 = b_off64; t.cp = cp ? 1 : 0;
                t.nb = columns; t.row0 = 0; t.count = rows * columns;
                OsaSizes init{}, got{};
                init.first_oversize = ~0ull;
                SWH_HIP_CHECK(hipMemcpyAsync(sizes, &init, sizeof init, hipMemcpyHostToDevice, stream));
                f.sizes(scope, t, sizes, items);
                SWH_HIP_CHECK(hipMemcpyAsync(&got, sizes, sizeof got, hipMemcpyDeviceToHost, stream));
                SWH_HIP_CHECK(hipStreamSynchronize(stream));
                absorb(false);
                if (got.first_oversize != ~0ull)   // (the memory of a prepared tape changed since the lengths were read)
                    return fail(error, swh_unsupported_length_k, "a string of the slice at (%llu, %llu) grew over the limit: %s",
                                (unsigned long long)q0, (unsigned long long)c0, f.oversize);
                sum.cells += got.cells; symbols += got.symbols;
                const bool wide = !cp && got.a_total >= 16 && got.b_total >= 16;
                char *where[kScoredOutputs] = {};
                if (jaro) for (int o = 0; o < counts; ++o) where[o] = (char *)slice[o];
                else where[r.scorer == SWH_SCORER_OSA ? 0 : 1] = (char *)slice[0];   // the OSA distance; the LCS length
                f.launch(scope, t, items, got.items, where, columns * 8, bound, wide);
                absorb(true);

                ExtractLaunch x{};
                for (int o = 0; o < counts; ++o) x.counts[o] = slice[o];
                x.a = queries; x.b = candidates; x.a_off64 = a_off64; x.b_off64 = b_off64;
                x.rows = rows; x.columns = columns; x.row_first = q0; x.col_first = c0;
                x.scorer = r.scorer; x.k = r.k; x.emit = c0 + columns == nc ? 1u : 0u;
                x.cutoff_bits = cutoff_bits; x.prefix_weight = r.prefix_weight;
                x.lists = lists; x.indices = ind; x.scores = sco;
                launch_extract_select(scope, x);
                absorb(false);
            }
        }
        if (!dev_i) SWH_HIP_CHECK(hipMemcpyAsync(r.indices, ind, index_bytes, hipMemcpyDeviceToHost, stream));
        if (!dev_s) SWH_HIP_CHECK(hipMemcpyAsync(r.scores, sco, score_bytes, hipMemcpyDeviceToHost, stream));
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        scope->summary_pending = false;
        scope->stamps_pending = false;
        sum.bytes = (cp ? 4 : 1) * symbols + index_bytes + score_bytes;
        snprintf(sum.dominant_name, sizeof sum.dominant_name, "extract_select/%s", scoring_name);
        scope->last_timing = sum;
        if (scope->profiling) add_to_totals(scope->totals, sum);
        return swh_success_k;
    });
}

static swh_status_t extract_checks(swh_levenshtein_t e, swh_scope_t s, int scorer, size_t k, uint64_t cutoff_bits, uint64_t prefix_weight_bits,
                                   size_t queries, size_t candidates, const uint32_t *indices, const void *scores, ExtractRequest &request,
                                   const char **error) {
    const swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    const Engine *engine = (const Engine *)e;
    if (engine->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (scorer < SWH_SCORER_OSA || scorer > SWH_SCORER_JARO_WINKLER) return fail(error, swh_invalid_argument_k, "scorer must be one of SWH_SCORER_*");
    if (k < 1 || k > SWH_TOPK_MAX) return fail(error, swh_invalid_argument_k, "k must lie in [1, SWH_TOPK_MAX]");
    double cutoff, prefix_weight;
    memcpy(&cutoff, &cutoff_bits, sizeof cutoff);
    memcpy(&prefix_weight, &prefix_weight_bits, sizeof prefix_weight);
    if (!(cutoff >= 0.0)) return fail(error, swh_invalid_argument_k, "the cutoff must be a non-negative number (or +infinity), not NaN");
    if (scorer == SWH_SCORER_JARO_WINKLER && !(prefix_weight >= 0.0 && prefix_weight <= 0.25))
        return fail(error, swh_invalid_argument_k, "the prefix weight must lie in [0, 0.25]");
    if (!engine->unit_costs)
        return fail(error, swh_not_implemented_k, "the score search is called on a unit-cost engine (match 0, mismatch 1, open 1, extend 1)");
    if (candidates >= 0xFFFFFFFFull) return fail(error, swh_unsupported_length_k, "2^32 - 1 candidates or more");
    if (queries && (!indices || !scores)) return fail(error, swh_invalid_argument_k, "null output pointer");
    request = ExtractRequest{scorer, (uint32_t)k, cutoff == 0.0 ? 0.0 : cutoff, prefix_weight, (uint32_t *)indices, (void *)scores};   // (-0.0: +0.0)
    return swh_success_k;
}

static swh_status_t extract_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *q, const swh_tape_u64_t *c, bool utf8, int scorer,
                                  size_t k, uint64_t cutoff_bits, uint64_t prefix_weight_bits, uint32_t *indices, void *scores, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (!q) return fail(error, swh_invalid_argument_k, "null tape");
    ExtractRequest request{};
    status = extract_checks(e, s, scorer, k, cutoff_bits, prefix_weight_bits, q->count, (c ? c : q)->count, indices, scores, request, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    if (q->count == 0) return swh_success_k;
    if ((status = call.prepare(q, c, utf8, true, true, error)) != swh_success_k) return status;
    return extract_run(call.scope, call.pair, request, error);
}
swh_status_t swh_levenshtein_extract_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries, const swh_tape_u64_t *candidates,
                                             int scorer, size_t k, uint64_t cutoff_bits, uint64_t prefix_weight_bits, uint32_t *indices,
                                             void *scores, const char **error) {
    return extract_tapes(e, s, queries, candidates, false, scorer, k, cutoff_bits, prefix_weight_bits, indices, scores, error);
}
swh_status_t swh_levenshtein_utf8_extract_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries,
                                                  const swh_tape_u64_t *candidates, int scorer, size_t k, uint64_t cutoff_bits,
                                                  uint64_t prefix_weight_bits, uint32_t *indices, void *scores, const char **error) {
    return extract_tapes(e, s, queries, candidates, true, scorer, k, cutoff_bits, prefix_weight_bits, indices, scores, error);
}
swh_status_t swh_levenshtein_extract_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *queries,
                                              const swh_prepared_view_t *candidates, int scorer, size_t k, uint64_t cutoff_bits,
                                              uint64_t prefix_weight_bits, uint32_t *indices, void *scores, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.views(queries, candidates, true, error)) != swh_success_k) return status;
    ExtractRequest request{};
    status = extract_checks(e, s, scorer, k, cutoff_bits, prefix_weight_bits, call.pair.a_count, call.pair.b_count, indices, scores, request, error);
    if (status != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return extract_run(call.scope, call.pair, request, error);
}

}  // extern "C"
