// api.hpp -- what api.hip (scope lifetime, timing, prepared tapes, the engine-call path) shares with two_tape.hip (the synchronous
// two-tape calls). Host code only; what is not defined in place is defined in api.hip.
#pragma once
#include "common.hpp"

namespace swh {

// error text: one slot per thread, whichever file refuses
__attribute__((format(printf, 3, 4))) swh_status_t fail(const char **error, swh_status_t status, const char *fmt, ...);
swh_status_t fail_hip(const char **error, const HipFailure &f);

void collect_timing(Scope *scope);
void add_to_totals(swh_timing_totals_t &totals, const swh_timing_t &call);
void harvest_timing(Scope *scope, bool complete);

// ---- scratch -------------------------------------------------------------------------------------
inline size_t pad(size_t n) { return (n + 255) & ~(size_t)255; }
struct Carver {
    char *base; size_t used, cap;
    template <typename T> T *take(size_t n) {
        char *p = base ? base + used : nullptr;
        used += pad(n * sizeof(T));
        return (T *)p;
    }
};
void ensure(char *&buf, size_t &cap, size_t need);
bool is_device_pointer(const void *p);
// Alignment scratch (align.hip) of every scope that ran an alignment: stored delta vectors, op slots, scans. Kept in a map in api.hip
// rather than in Scope so that common.hpp -- which every kernel family's profile stamp hashes -- stays as it is; freed with the scope.
struct AlignScratch { char *buf = nullptr; size_t bytes = 0; };
AlignScratch *call_scratch(const Scope *scope);   // the scope's own entry, made on first use (the lookup is locked)

// ---- one engine call ---------------------------------------------------------------------------
struct HostTape { const uint8_t *data; const void *offsets; size_t count; int off64; };
#define SWH_TAPE(t, w) HostTape{(t)->data, (const void *)(t)->offsets, (t)->count, (w)}

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
    // Side arrays of a byte tape (or null): per string two entries -- its first sixteen bytes [start, start + 16) and its last sixteen
    // [end - 16, end), positions outside the tape's bytes [0, total_bytes) as zero, the neighbouring strings' bytes included. What the
    // tiled kernel's planning needs of the strings, laid out so that it finds it by string number (tiled.hip: kSide). Only built where
    // that kernel can be chosen: prepare_tape has the conditions.
    const uint4 *side = nullptr;
    int token_form = -1;         // SWH_TOKENS_*: the normal form swh_tape_token_sort derived this tape in; -1 for every other tape
    std::vector<void *> owned;   // device buffers that go with the handle
};
// (declared here, not in common.hpp, which every kernel family's profile stamp hashes)
void launch_bitparallel_tiled_side(Scope *scope, const KernelArgs &args, uint64_t pairs, uint32_t longest_text, const uint4 *side_a, const uint4 *side_b);
swh_status_t prepare_tape(Scope *scope, const HostTape &tape, bool utf8, swh_prepared_t *out, const char **error);
void free_prepared(Prepared *p);

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
swh_status_t run_call_on(Scope *scope, const Engine *engine, const CallSpec &spec, const char **error);

// ---- prepared tapes in a call -------------------------------------------------------------------------------------------------
bool view_fits(const swh_prepared_view_t *view);
swh_status_t check_prepared_pair(const Scope *scope, const Prepared *pa, const Prepared *pb, const char **error);
// strings [first, first + count) of a prepared tape: its code points (`code_points` on a UTF-8 tape: u64 offsets) or its bytes
TapeRef prepared_view(const Prepared *p, bool code_points, size_t first, size_t count);
uint64_t read_offset(const void *offs, int off64, size_t i, bool device, hipStream_t stream);

// ---- the route decision (pick_route in api.hip has the table) ----------------------------------------------------------------------
// Which kernels a unit-cost Levenshtein call runs on.
enum Route { kRoutePlanned, kRouteTiled, kRouteDirectShort, kRouteShortTiled, kRouteCrossShort, kRouteAlignShort, kRouteAlignLong };
// What a call knows about its strings' lengths before it launches anything: a guarantee for prepared tapes, a belief from the scope's
// previous call (the kernels verify it), or -- a Levenshtein engine forced onto the tiled kernel -- that kernel's 2048 symbols.
struct Lengths {
    bool known = false, guaranteed = false;
    uint32_t la_max = 0, lb_max = 0;
    uint64_t prepared_mean_x16 = 0;   // prepared tapes: the longer mean string of the two whole tapes, bytes x 16
};
Lengths call_lengths(const Scope *scope, const Engine *engine, const CallSpec &spec, bool utf8);
struct RouteChoice {
    Route route = kRoutePlanned;
    uint32_t longest = 0;      // what the plan-free kernel is launched for
    bool align_wide = false;   // kRouteAlignShort on k_align_cross_wide (its alphabet condition is checked by the kernel)
};
RouteChoice pick_route(const Scope *scope, const Engine *engine, const CallSpec &spec, bool utf8, bool dev_out, const Lengths &len);

}  // namespace swh
