/* check_c -- the part of include/stringwars_amd.h that the C++ header does not wrap, called from C99 against expected arrays.
 *
 *   check_c <case file>
 *
 * The case file is written by tests/test_bindings.py from the suite's references. Format (little-endian, no padding): the 8 bytes
 * "SWCASE1\0", a u32 array count, then per array a u32 name length, the name, a u32 dtype code (0 u8, 1 u32, 2 u64, 3 i32, 4 i64,
 * 5 i8), a u64 element count and the elements. Arrays read here: the tapes <name>.data (u8) / <name>.off (u64) for b.pa, b.pb, u.pa,
 * u.pb, b.q, b.c, nw.pa, nw.pb, nw.q, nw.c, long.a, long.b, bad.a, bad.b; b.lev, u.lev, b.osa, b.indel, b.lcs, b.jaro_m / _t / _p (u32);
 * b.x.jaro_m / _t / _p (u64); nw.classes, nw.costs, nw.matrix; <nw|sw>.classes.linear.<pairs|cross|self>.
 *
 * One line per check on stdout, `<name>: ok` or what differs. Outputs are filled with the sentinel byte 0xA5 before a call; a refused
 * call must leave them so. Exit status 0 when every line is ok. With no device visible every entry point of the header is called
 * once with null handles (`nodevice.<symbol>` lines): the documented status, a message where the call has an `error` parameter, and
 * untouched outputs. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "stringwars_amd.h"
#include "stringwars_amd_harness.h"

#define SENTINEL 0xA5
#define MAX_ARRAYS 1024

typedef struct { char name[64]; uint32_t dtype; uint64_t count; unsigned char *bytes; } array_t;
static const size_t k_width[6] = {1, 4, 8, 4, 8, 1};
static array_t g_arrays[MAX_ARRAYS];
static size_t g_array_count = 0;
static int g_failures = 0;
static char g_message[256];

static void die(const char *what, const char *name) {
    fprintf(stderr, "check_c: %s %s\n", what, name);
    exit(3);
}

static void load_case(const char *path) {
    FILE *in = fopen(path, "rb");
    char magic[8];
    uint32_t arrays = 0, i;
    if (!in) die("cannot open", path);
    if (fread(magic, 1, 8, in) != 8 || fread(&arrays, 4, 1, in) != 1 || memcmp(magic, "SWCASE1\0", 8) != 0) die("not a case file:", path);
    if (arrays > MAX_ARRAYS) die("too many arrays in", path);
    for (i = 0; i < arrays; ++i) {
        array_t *a = &g_arrays[g_array_count];
        uint32_t length = 0;
        size_t bytes;
        if (fread(&length, 4, 1, in) != 1 || length >= sizeof a->name || fread(a->name, 1, length, in) != length) die("bad array name in", path);
        a->name[length] = 0;
        if (fread(&a->dtype, 4, 1, in) != 1 || fread(&a->count, 8, 1, in) != 1 || a->dtype > 5) die("bad array header:", a->name);
        bytes = (size_t)a->count * k_width[a->dtype];
        a->bytes = (unsigned char *)malloc(bytes + 8);
        if (!a->bytes || fread(a->bytes, 1, bytes, in) != bytes) die("short case file at", a->name);
        ++g_array_count;
    }
    fclose(in);
}

static void free_case(void) {
    size_t i;
    for (i = 0; i < g_array_count; ++i) free(g_arrays[i].bytes);
}

static const void *arr(const char *name, size_t width, size_t *count) {
    size_t i;
    for (i = 0; i < g_array_count; ++i)
        if (strcmp(g_arrays[i].name, name) == 0) {
            if (k_width[g_arrays[i].dtype] != width) die("another element width:", name);
            if (count) *count = (size_t)g_arrays[i].count;
            return g_arrays[i].bytes;
        }
    die("the case file has no array", name);
    return NULL;
}

static swh_tape_u64_t tape64(const char *name) {
    char key[80];
    size_t entries = 0;
    swh_tape_u64_t t;
    snprintf(key, sizeof key, "%s.off", name);
    t.offsets = (const uint64_t *)arr(key, 8, &entries);
    snprintf(key, sizeof key, "%s.data", name);
    t.data = (const uint8_t *)arr(key, 1, NULL);
    t.count = entries - 1;
    return t;
}

/* the same tape with 32-bit offsets; the caller frees `*offsets` */
static swh_tape_u32_t tape32(const char *name, uint32_t **offsets) {
    swh_tape_u64_t wide = tape64(name);
    swh_tape_u32_t t;
    size_t i;
    *offsets = (uint32_t *)malloc((wide.count + 1) * sizeof(uint32_t));
    if (!*offsets) die("out of memory for", name);
    for (i = 0; i <= wide.count; ++i) (*offsets)[i] = (uint32_t)wide.offsets[i];
    t.data = wide.data; t.offsets = *offsets; t.count = wide.count;
    return t;
}

static void report(const char *name, const char *problem) {
    printf("%s: %s\n", name, problem ? problem : "ok");
    if (problem) ++g_failures;
}

/* a sentinel-filled buffer of `bytes` and a guard element behind it */
static void *fresh(size_t bytes) {
    void *p = malloc(bytes + 16);
    if (!p) die("out of memory", "");
    memset(p, SENTINEL, bytes + 16);
    return p;
}

static const char *untouched(const char *what, const void *buffer, size_t bytes) {
    const unsigned char *p = (const unsigned char *)buffer;
    size_t i;
    for (i = 0; i < bytes; ++i)
        if (p[i] != SENTINEL) {
            snprintf(g_message, sizeof g_message, "%s: byte %lu was written, the call must leave it at its sentinel", what, (unsigned long)i);
            return g_message;
        }
    return NULL;
}

/* NULL when the n elements of `elem` bytes, `stride` bytes apart, equal want[0 .. n), and every other byte of the `bytes + 16` of a
 * fresh() buffer still holds the sentinel; else the first difference */
static const char *compare(const char *what, const void *got, size_t stride, size_t elem, size_t n, const void *want, size_t bytes) {
    const unsigned char *g = (const unsigned char *)got, *w = (const unsigned char *)want;
    size_t i, b;
    for (i = 0; i < n; ++i) {
        if (memcmp(g + i * stride, w + i * elem, elem) != 0) {
            uint64_t gv = 0, wv = 0;
            memcpy(&gv, g + i * stride, elem);
            memcpy(&wv, w + i * elem, elem);
            snprintf(g_message, sizeof g_message, "%s: first difference at index %lu: got %llu want %llu", what, (unsigned long)i,
                     (unsigned long long)gv, (unsigned long long)wv);
            return g_message;
        }
        for (b = i * stride + elem; b < (i + 1) * stride && b < bytes + 16; ++b)
            if (g[b] != SENTINEL) {
                snprintf(g_message, sizeof g_message, "%s: padding byte %lu behind element %lu was written", what, (unsigned long)(b - i * stride), (unsigned long)i);
                return g_message;
            }
    }
    for (b = n * stride; b < bytes + 16; ++b)
        if (g[b] != SENTINEL) {
            snprintf(g_message, sizeof g_message, "%s: byte %lu past the end was written", what, (unsigned long)(b - n * stride));
            return g_message;
        }
    return NULL;
}

static const char *failed(const char *what, swh_status_t status, const char *error) {
    snprintf(g_message, sizeof g_message, "%s: status %d: %s", what, (int)status, error ? error : "");
    return g_message;
}

/* a refusal: the documented status, a message, and outputs (sentinel-filled, `bytes` long) left alone */
static void refused(const char *name, swh_status_t status, swh_status_t want, const char *error, const void *outputs, size_t bytes) {
    if (status != want) {
        snprintf(g_message, sizeof g_message, "status %d, the header documents %d (%s)", (int)status, (int)want, error ? error : "");
        report(name, g_message);
    } else if (!error || !*error) report(name, "no error message");
    else report(name, untouched("outputs", outputs, bytes));
}

/* ---- with a device -------------------------------------------------------------------------------------------------------------------- */
#define MUST(call) do { const swh_status_t status__ = (call); if (status__ != swh_success_k) { report(#call, failed("setup", status__, err)); return; } } while (0)

static void with_a_device(void) {
    const char *err = NULL;
    swh_scope_t scope = NULL;
    swh_levenshtein_t lev = NULL;
    swh_nw_t nw = NULL;
    swh_sw_t sw = NULL;
    swh_prepared_t prepared[6] = {NULL, NULL, NULL, NULL, NULL, NULL};
    swh_prepared_view_t view[6];
    const swh_tape_u64_t ba = tape64("b.pa"), bb = tape64("b.pb"), bq = tape64("b.q"), bc = tape64("b.c");
    const swh_tape_u64_t na = tape64("nw.pa"), nb = tape64("nw.pb"), nq = tape64("nw.q"), nc = tape64("nw.c");
    const swh_tape_u64_t long_a = tape64("long.a"), long_b = tape64("long.b"), bad_a = tape64("bad.a"), bad_b = tape64("bad.b");
    const size_t n = ba.count, pairs = na.count;
    const uint32_t *lev_want = (const uint32_t *)arr("b.lev", 4, NULL);
    const int32_t *nw_want = (const int32_t *)arr("nw.classes.linear.pairs", 4, NULL), *sw_want = (const int32_t *)arr("sw.classes.linear.pairs", 4, NULL);
    swh_status_t status;
    size_t i;

    MUST(swh_scope_init_gpu(0, &scope, &err));
    MUST(swh_levenshtein_init(scope, 0, 1, 1, 1, &lev, &err));
    MUST(swh_nw_init_classes(scope, (const uint8_t *)arr("nw.classes", 1, NULL), (const int8_t *)arr("nw.costs", 1, NULL), -4, -4, &nw, &err));
    MUST(swh_sw_init_classes(scope, (const uint8_t *)arr("nw.classes", 1, NULL), (const int8_t *)arr("nw.costs", 1, NULL), -4, -4, &sw, &err));

    {   /* the *_u32tape entry points against the same expected arrays as their *_u64tape twins */
        uint32_t *oa, *ob, *oua, *oub, *ona, *onb;
        const swh_tape_u32_t a32 = tape32("b.pa", &oa), b32 = tape32("b.pb", &ob), ua32 = tape32("u.pa", &oua), ub32 = tape32("u.pb", &oub);
        const swh_tape_u32_t na32 = tape32("nw.pa", &ona), nb32 = tape32("nw.pb", &onb);
        uint32_t *out = (uint32_t *)fresh(n * 4), *twin = (uint32_t *)fresh(n * 4);
        status = swh_levenshtein_pairs_u32tape(lev, scope, &a32, &b32, SWH_UNBOUNDED, out, 0, &err);
        if (status == swh_success_k) status = swh_levenshtein_pairs_u64tape(lev, scope, &ba, &bb, SWH_UNBOUNDED, twin, 0, &err);
        report("u32tape.levenshtein_pairs", status != swh_success_k ? failed("call", status, err)
               : compare("u32 offsets", out, 4, 4, n, lev_want, n * 4) ? g_message : compare("u64 offsets", twin, 4, 4, n, lev_want, n * 4));
        memset(out, SENTINEL, n * 4 + 16);
        status = swh_levenshtein_utf8_pairs_u32tape(lev, scope, &ua32, &ub32, SWH_UNBOUNDED, out, 4, &err);
        report("u32tape.levenshtein_utf8_pairs", status != swh_success_k ? failed("call", status, err) : compare("distances", out, 4, 4, n, arr("u.lev", 4, NULL), n * 4));
        memset(out, SENTINEL, n * 4 + 16);
        status = swh_nw_pairs_u32tape(nw, scope, &na32, &nb32, (int32_t *)out, 0, &err);
        report("u32tape.nw_pairs", status != swh_success_k ? failed("call", status, err) : compare("scores", out, 4, 4, pairs, nw_want, pairs * 4));
        memset(out, SENTINEL, n * 4 + 16);
        status = swh_sw_pairs_u32tape(sw, scope, &na32, &nb32, (int32_t *)out, 0, &err);
        report("u32tape.sw_pairs", status != swh_success_k ? failed("call", status, err) : compare("scores", out, 4, 4, pairs, sw_want, pairs * 4));
        {   /* swh_tape_prepare_u32: device copies are made, so the host offsets may go once the tapes are prepared */
            swh_prepared_t pa = NULL, pb = NULL;
            swh_prepared_info_t info;
            memset(&info, 0, sizeof info);
            memset(out, SENTINEL, n * 4 + 16);
            status = swh_tape_prepare_u32(scope, &a32, 0, &pa, &err);
            if (status == swh_success_k) status = swh_tape_prepare_u32(scope, &b32, 0, &pb, &err);
            if (status == swh_success_k) {
                swh_prepared_view_t va, vb;
                va.tape = pa; va.first = 0; va.count = n;
                vb.tape = pb; vb.first = 0; vb.count = n;
                status = swh_levenshtein_pairs_prepared(lev, scope, &va, &vb, SWH_UNBOUNDED, out, 0, &err);
            }
            if (status == swh_success_k) status = swh_prepared_info(pa, &info);
            report("u32tape.prepare_u32", status != swh_success_k ? failed("call", status, err)
                   : info.count != n || info.bytes != ba.offsets[n] || info.utf8 != 0 ? "swh_prepared_info differs from the tape"
                   : compare("distances", out, 4, 4, n, lev_want, n * 4));
            swh_prepared_free(pa);
            swh_prepared_free(pb);
        }
        free(out); free(twin); free(oa); free(ob); free(oua); free(oub); free(ona); free(onb);
    }

    {   /* swh_nw_*_prepared / swh_sw_*_prepared; the byte tapes b.pa / b.pb prepared here serve the pipelined check below */
        const swh_tape_u64_t *tapes[6];
        const char *names[6] = {"prepared.nw_pairs", "prepared.nw_cross", "prepared.sw_pairs", "prepared.sw_cross", "", ""};
        tapes[0] = &na; tapes[1] = &nb; tapes[2] = &nq; tapes[3] = &nc; tapes[4] = &ba; tapes[5] = &bb;
        for (i = 0; i < 6; ++i) {
            MUST(swh_tape_prepare_u64(scope, tapes[i], 0, &prepared[i], &err));
            view[i].tape = prepared[i]; view[i].first = 0; view[i].count = tapes[i]->count;
        }
        for (i = 0; i < 2; ++i) {
            const char *prefix = i ? "sw" : "nw";
            char key[64];
            const size_t cells = nq.count * nc.count, self_cells = nq.count * nq.count;
            int32_t *out = (int32_t *)fresh(pairs * 4);
            ptrdiff_t *matrix = (ptrdiff_t *)fresh(cells * 8), *self = (ptrdiff_t *)fresh(self_cells * 8);
            status = i ? swh_sw_pairs_prepared(sw, scope, &view[0], &view[1], out, 0, &err) : swh_nw_pairs_prepared(nw, scope, &view[0], &view[1], out, 0, &err);
            report(names[2 * i], status != swh_success_k ? failed("call", status, err) : compare("scores", out, 4, 4, pairs, i ? sw_want : nw_want, pairs * 4));
            status = i ? swh_sw_cross_prepared(sw, scope, &view[2], &view[3], matrix, 0, &err) : swh_nw_cross_prepared(nw, scope, &view[2], &view[3], matrix, 0, &err);
            if (status == swh_success_k)
                status = i ? swh_sw_cross_prepared(sw, scope, &view[2], NULL, self, 0, &err) : swh_nw_cross_prepared(nw, scope, &view[2], NULL, self, 0, &err);
            snprintf(key, sizeof key, "%s.classes.linear.cross", prefix);
            if (status == swh_success_k && compare("matrix", matrix, 8, 8, cells, arr(key, 8, NULL), cells * 8)) report(names[2 * i + 1], g_message);
            else {
                snprintf(key, sizeof key, "%s.classes.linear.self", prefix);
                report(names[2 * i + 1], status != swh_success_k ? failed("call", status, err) : compare("self-product", self, 8, 8, self_cells, arr(key, 8, NULL), self_cells * 8));
            }
            free(out); free(matrix); free(self);
        }
    }

    {   /* out_stride_bytes: 8 between results, and 12 for the Jaro pairs ("a multiple of 4") */
        unsigned char *out = (unsigned char *)fresh(n * 12), *second = (unsigned char *)fresh(n * 12), *third = (unsigned char *)fresh(n * 12);
        status = swh_levenshtein_pairs_u64tape(lev, scope, &ba, &bb, SWH_UNBOUNDED, (uint32_t *)out, 8, &err);
        report("stride8.levenshtein_pairs", status != swh_success_k ? failed("call", status, err) : compare("distances", out, 8, 4, n, lev_want, n * 12));
        memset(out, SENTINEL, n * 12 + 16);
        status = swh_levenshtein_osa_pairs_u64tape(lev, scope, &ba, &bb, SWH_UNBOUNDED, (uint32_t *)out, 8, &err);
        report("stride8.osa_pairs", status != swh_success_k ? failed("call", status, err) : compare("distances", out, 8, 4, n, arr("b.osa", 4, NULL), n * 12));
        memset(out, SENTINEL, n * 12 + 16);
        status = swh_levenshtein_lcs_pairs_u64tape(lev, scope, &ba, &bb, SWH_UNBOUNDED, (uint32_t *)out, (uint32_t *)second, 8, &err);
        report("stride8.lcs_pairs", status != swh_success_k ? failed("call", status, err)
               : compare("indel", out, 8, 4, n, arr("b.indel", 4, NULL), n * 12) ? g_message : compare("lcs", second, 8, 4, n, arr("b.lcs", 4, NULL), n * 12));
        memset(out, SENTINEL, n * 12 + 16);
        status = swh_nw_pairs_u64tape(nw, scope, &na, &nb, (int32_t *)out, 8, &err);
        report("stride8.nw_pairs", status != swh_success_k ? failed("call", status, err) : compare("scores", out, 8, 4, pairs, nw_want, n * 12));
        memset(out, SENTINEL, n * 12 + 16);
        memset(second, SENTINEL, n * 12 + 16);
        status = swh_levenshtein_jaro_pairs_u64tape(lev, scope, &ba, &bb, (uint32_t *)out, (uint32_t *)second, (uint32_t *)third, 12, &err);
        report("stride12.jaro_pairs", status != swh_success_k ? failed("call", status, err)
               : compare("matches", out, 12, 4, n, arr("b.jaro_m", 4, NULL), n * 12) ? g_message
               : compare("transpositions", second, 12, 4, n, arr("b.jaro_t", 4, NULL), n * 12) ? g_message
               : compare("prefix", third, 12, 4, n, arr("b.jaro_p", 4, NULL), n * 12));
        free(out); free(second); free(third);
    }

    {   /* outputs in swh_device_alloc memory (read back with swh_copy_to_host) and in swh_unified_alloc memory */
        const size_t bytes = n * 4 + 16, cells = bq.count * bc.count, matrix_bytes = cells * 8 + 16;
        void *device = NULL, *unified = NULL, *matrices[3] = {NULL, NULL, NULL};
        uint32_t *host = (uint32_t *)fresh(n * 4), *back = (uint32_t *)malloc(bytes);
        unsigned char *matrix_fill = (unsigned char *)fresh(cells * 8), *matrix_back = (unsigned char *)malloc(matrix_bytes);
        const char *keys[3] = {"b.x.jaro_m", "b.x.jaro_t", "b.x.jaro_p"};
        const char *problem = NULL;
        MUST(swh_device_alloc(scope, bytes, &device, &err));
        MUST(swh_unified_alloc(scope, bytes, &unified, &err));
        MUST(swh_copy_to_device(scope, device, host, bytes, &err));
        status = swh_levenshtein_pairs_u64tape(lev, scope, &ba, &bb, SWH_UNBOUNDED, (uint32_t *)device, 0, &err);
        if (status == swh_success_k) status = swh_copy_to_host(scope, back, device, bytes, &err);
        report("device_alloc.levenshtein_pairs", status != swh_success_k ? failed("call", status, err) : compare("distances", back, 4, 4, n, lev_want, n * 4));
        memset(unified, SENTINEL, bytes);
        status = swh_levenshtein_pairs_u64tape(lev, scope, &ba, &bb, SWH_UNBOUNDED, (uint32_t *)unified, 0, &err);
        report("unified_alloc.levenshtein_pairs", status != swh_success_k ? failed("call", status, err) : compare("distances", unified, 4, 4, n, lev_want, n * 4));
        for (i = 0; i < 3; ++i) {
            MUST(swh_device_alloc(scope, matrix_bytes, &matrices[i], &err));
            MUST(swh_copy_to_device(scope, matrices[i], matrix_fill, matrix_bytes, &err));
        }
        status = swh_levenshtein_jaro_cross_u64tape(lev, scope, &bq, &bc, (size_t *)matrices[0], (size_t *)matrices[1], (size_t *)matrices[2], 0, &err);
        for (i = 0; i < 3 && status == swh_success_k && !problem; ++i) {
            status = swh_copy_to_host(scope, matrix_back, matrices[i], matrix_bytes, &err);
            if (status == swh_success_k) problem = compare(keys[i], matrix_back, 8, 8, cells, arr(keys[i], 8, NULL), cells * 8);
        }
        report("device_alloc.jaro_cross", status != swh_success_k ? failed("call", status, err) : problem);

        /* asynchronous: the call only enqueues, swh_scope_synchronize makes the results visible */
        memset(unified, SENTINEL, bytes);
        MUST(swh_scope_set_async(scope, 1));
        status = swh_levenshtein_pairs_u64tape(lev, scope, &ba, &bb, SWH_UNBOUNDED, (uint32_t *)unified, 0, &err);
        if (status == swh_success_k) status = swh_scope_synchronize(scope, &err);
        report("async.synchronize", status != swh_success_k ? failed("call", status, err) : compare("distances", unified, 4, 4, n, lev_want, n * 4));
        MUST(swh_scope_set_async(scope, 0));
        /* pipelined: swh_scope_join orders the scope's stream behind the latest call; the copy back runs on that stream */
        MUST(swh_copy_to_device(scope, device, host, bytes, &err));
        MUST(swh_scope_set_pipelined(scope, 1, &err));
        status = swh_levenshtein_pairs_prepared(lev, scope, &view[4], &view[5], SWH_UNBOUNDED, (uint32_t *)device, 0, &err);
        if (status == swh_success_k) status = swh_scope_join(scope, &err);
        if (status == swh_success_k) status = swh_copy_to_host(scope, back, device, bytes, &err);
        report("pipelined.join", status != swh_success_k ? failed("call", status, err) : compare("distances", back, 4, 4, n, lev_want, n * 4));
        MUST(swh_scope_set_pipelined(scope, 0, &err));
        for (i = 0; i < 3; ++i) swh_device_free(scope, matrices[i]);
        swh_device_free(scope, device);
        swh_unified_free(scope, unified);
        free(host); free(back); free(matrix_fill); free(matrix_back);
    }

    {   /* swh_scope_describe into a buffer that is too short; swh_scope_forget, then the same call with the same result */
        char full[1024], brief[64];
        uint32_t *first = (uint32_t *)fresh(n * 4), *again = (uint32_t *)fresh(n * 4);
        memset(brief, SENTINEL, sizeof brief);
        status = swh_scope_describe(scope, full, sizeof full);
        if (status == swh_success_k) status = swh_scope_describe(scope, brief, 16);
        report("describe.short", status != swh_success_k ? failed("call", status, NULL)
               : strlen(full) < 40 ? "the full description is implausibly short"
               : memchr(brief, 0, 16) == NULL ? "not NUL-terminated within the capacity"
               : strlen(brief) != 15 || strncmp(brief, full, 15) != 0 ? "not the first capacity - 1 characters of the description"
               : untouched("bytes past the capacity", brief + 16, sizeof brief - 16));
        status = swh_levenshtein_pairs_u64tape(lev, scope, &ba, &bb, SWH_UNBOUNDED, first, 0, &err);
        if (status == swh_success_k) status = swh_scope_forget(scope);
        if (status == swh_success_k) status = swh_scope_describe(scope, full, sizeof full);
        if (status == swh_success_k && !strstr(full, "lengths_believed=0")) report("forget.again", "the scope still believes the last call's lengths");
        else {
            if (status == swh_success_k) status = swh_levenshtein_pairs_u64tape(lev, scope, &ba, &bb, SWH_UNBOUNDED, again, 0, &err);
            report("forget.again", status != swh_success_k ? failed("call", status, err)
                   : compare("before", first, 4, 4, n, lev_want, n * 4) ? g_message : compare("after", again, 4, 4, n, lev_want, n * 4));
        }
        free(first); free(again);
    }

    {   /* refusals: the documented status, a message, the outputs left at their sentinel */
        const size_t bytes = 4096 * 8;
        unsigned char *o = (unsigned char *)fresh(bytes);
        uint32_t *o1 = (uint32_t *)o, *o2 = (uint32_t *)(o + 8192), *o3 = (uint32_t *)(o + 16384);
        size_t *offsets = (size_t *)(o + 24576);
        const uint32_t B = SWH_UNBOUNDED;
#define REFUSED(name, want, call) do { err = NULL; status = (call); refused(name, status, want, err, o, bytes + 16); memset(o, SENTINEL, bytes + 16); } while (0)
        /* a null engine beside a live scope, with a device present: swh_invalid_argument_k (the header's "Null handles") */
        REFUSED("refuse.null_engine.levenshtein_pairs", swh_invalid_argument_k, swh_levenshtein_pairs_u64tape(NULL, scope, &ba, &bb, B, o1, 0, &err));
        REFUSED("refuse.null_engine.topk", swh_invalid_argument_k, swh_levenshtein_topk_u64tape(NULL, scope, &bq, &bc, 1, B, o1, o2, &err));
        REFUSED("refuse.null_engine.infix", swh_invalid_argument_k, swh_levenshtein_infix_u64tape(NULL, scope, &ba, &bb, B, o1, o2, o3, &err));
        REFUSED("refuse.null_engine.osa_pairs", swh_invalid_argument_k, swh_levenshtein_osa_pairs_u64tape(NULL, scope, &ba, &bb, B, o1, 0, &err));
        /* tapes of different counts in a pairwise call */
        REFUSED("refuse.counts.levenshtein_pairs", swh_invalid_argument_k, swh_levenshtein_pairs_u64tape(lev, scope, &bq, &bc, B, o1, 0, &err));
        REFUSED("refuse.counts.align", swh_invalid_argument_k, swh_levenshtein_align_u64tape(lev, scope, &bq, &bc, B, o1, offsets, (char *)o2, 8192, &err));
        REFUSED("refuse.counts.infix", swh_invalid_argument_k, swh_levenshtein_infix_u64tape(lev, scope, &bq, &bc, B, o1, o2, o3, &err));
        REFUSED("refuse.counts.osa_pairs", swh_invalid_argument_k, swh_levenshtein_osa_pairs_u64tape(lev, scope, &bq, &bc, B, o1, 0, &err));
        REFUSED("refuse.counts.lcs_pairs", swh_invalid_argument_k, swh_levenshtein_lcs_pairs_u64tape(lev, scope, &bq, &bc, B, o1, o2, 0, &err));
        REFUSED("refuse.counts.jaro_pairs", swh_invalid_argument_k, swh_levenshtein_jaro_pairs_u64tape(lev, scope, &bq, &bc, o1, o2, o3, 0, &err));
        REFUSED("refuse.counts.nw_pairs", swh_invalid_argument_k, swh_nw_pairs_u64tape(nw, scope, &nq, &nc, (int32_t *)o1, 0, &err));
        /* a stray continuation byte in a UTF-8 call */
        REFUSED("refuse.utf8.levenshtein_pairs", swh_invalid_utf8_k, swh_levenshtein_utf8_pairs_u64tape(lev, scope, &bad_a, &bad_b, B, o1, 0, &err));
        {
            swh_prepared_t handle = NULL;
            REFUSED("refuse.utf8.prepare", swh_invalid_utf8_k, swh_tape_prepare_u64(scope, &bad_a, 1, &handle, &err));
            if (handle) { report("refuse.utf8.prepare.handle", "a handle was returned with the refusal"); swh_prepared_free(handle); }
        }
        REFUSED("refuse.utf8.align", swh_invalid_utf8_k, swh_levenshtein_utf8_align_u64tape(lev, scope, &bad_a, &bad_b, B, o1, offsets, (char *)o2, 8192, &err));
        REFUSED("refuse.utf8.infix", swh_invalid_utf8_k, swh_levenshtein_utf8_infix_u64tape(lev, scope, &bad_a, &bad_b, B, o1, o2, o3, &err));
        REFUSED("refuse.utf8.osa_pairs", swh_invalid_utf8_k, swh_levenshtein_utf8_osa_pairs_u64tape(lev, scope, &bad_a, &bad_b, B, o1, 0, &err));
        REFUSED("refuse.utf8.lcs_pairs", swh_invalid_utf8_k, swh_levenshtein_utf8_lcs_pairs_u64tape(lev, scope, &bad_a, &bad_b, B, o1, o2, 0, &err));
        REFUSED("refuse.utf8.jaro_pairs", swh_invalid_utf8_k, swh_levenshtein_utf8_jaro_pairs_u64tape(lev, scope, &bad_a, &bad_b, o1, o2, o3, 0, &err));
        REFUSED("refuse.utf8.topk", swh_invalid_utf8_k, swh_levenshtein_utf8_topk_u64tape(lev, scope, &bad_a, &bad_b, 2, B, o1, o2, &err));
        REFUSED("refuse.utf8.within", swh_invalid_utf8_k, swh_levenshtein_utf8_within_u64tape(lev, scope, &bad_a, &bad_b, 1, offsets, o1, o2, 1024, &err));
        /* one symbol more than the call takes: SWH_INFIX_MAX_PATTERN + 1, SWH_OSA_MAX_SHORTER + 1, SWH_LCS_MAX_SHORTER + 1, SWH_JARO_MAX_LENGTH + 1 */
        if (long_a.offsets[1] != SWH_INFIX_MAX_PATTERN + 1 || long_a.offsets[1] != SWH_OSA_MAX_SHORTER + 1 || long_a.offsets[1] != SWH_LCS_MAX_SHORTER + 1 ||
            long_a.offsets[1] != SWH_JARO_MAX_LENGTH + 1 || long_b.offsets[1] != long_a.offsets[1])
            report("refuse.length.inputs", "the long pair is not one symbol over every limit");
        REFUSED("refuse.length.infix", swh_unsupported_length_k, swh_levenshtein_infix_u64tape(lev, scope, &long_a, &long_b, B, o1, o2, o3, &err));
        REFUSED("refuse.length.osa_pairs", swh_unsupported_length_k, swh_levenshtein_osa_pairs_u64tape(lev, scope, &long_a, &long_b, B, o1, 0, &err));
        REFUSED("refuse.length.lcs_pairs", swh_unsupported_length_k, swh_levenshtein_lcs_pairs_u64tape(lev, scope, &long_a, &long_b, B, o1, o2, 0, &err));
        REFUSED("refuse.length.jaro_pairs", swh_unsupported_length_k, swh_levenshtein_jaro_pairs_u64tape(lev, scope, &long_a, &long_b, o1, o2, o3, 0, &err));
#undef REFUSED
        free(o);
    }

    for (i = 0; i < 6; ++i) swh_prepared_free(prepared[i]);
    swh_sw_free(sw);
    swh_nw_free(nw);
    swh_levenshtein_free(lev);
    swh_scope_free(scope);
}

static void introspection(void) {
    char want[32];
    const char *tokens[] = {"gfx950", "hip", "utf8", "topk", "within", "align", "infix", "osa", "lcs", "jaro"};
    const char *capabilities = swh_capabilities();
    char padded[1024];
    size_t i;
    snprintf(want, sizeof want, "%d.%d.%d", SWH_VERSION_MAJOR, SWH_VERSION_MINOR, SWH_VERSION_PATCH);
    report("version", swh_version() && strcmp(swh_version(), want) == 0 ? NULL : "swh_version() is not SWH_VERSION_MAJOR.MINOR.PATCH");
    snprintf(padded, sizeof padded, ",%s,", capabilities ? capabilities : "");
    for (i = 0; i < sizeof tokens / sizeof tokens[0]; ++i) {
        char token[32];
        snprintf(token, sizeof token, ",%s,", tokens[i]);
        if (!strstr(padded, token)) {
            snprintf(g_message, sizeof g_message, "swh_capabilities() lacks %s", tokens[i]);
            report("capabilities", g_message);
            return;
        }
    }
    report("capabilities", NULL);
}

/* ---- without a device: every entry point once, null handles ------------------------------------------------------------------------------ */
static unsigned char g_outputs[4][256];   /* what the calls are given to write to */

static void nodevice(const char *symbol, int status, int want, int has_error, const char *error) {
    char name[96];
    size_t i;
    const char *problem = NULL;
    snprintf(name, sizeof name, "nodevice.%s", symbol);
    if (status != want) {
        snprintf(g_message, sizeof g_message, "status %d, the header documents %d (%s)", status, want, error ? error : "");
        problem = g_message;
    } else if (has_error && want != swh_success_k && (!error || !*error)) problem = "no error message";
    for (i = 0; i < 4 && !problem; ++i) problem = untouched("outputs", g_outputs[i], sizeof g_outputs[i]);
    report(name, problem);
    memset(g_outputs, SENTINEL, sizeof g_outputs);
}

#define ND(symbol, want, arguments) do { int status__; err = NULL; status__ = (int)symbol arguments; nodevice(#symbol, status__, (int)(want), 1, err); } while (0)
#define ND_PLAIN(symbol, want, arguments) do { int status__ = (int)symbol arguments; nodevice(#symbol, status__, (int)(want), 0, NULL); } while (0)

static void without_a_device(void) {
    const char *err = NULL;
    const swh_status_t none = swh_no_device_k, bad = swh_invalid_argument_k, fine = swh_success_k;
    uint32_t *offsets32 = NULL;
    const swh_tape_u64_t a = tape64("bad.a"), b = tape64("bad.b");
    const swh_tape_u32_t a32 = tape32("bad.a", &offsets32), b32 = a32;
    swh_prepared_view_t v;
    uint32_t *o1 = (uint32_t *)g_outputs[0], *o2 = (uint32_t *)g_outputs[1], *o3 = (uint32_t *)g_outputs[2];
    size_t *z1 = (size_t *)g_outputs[0], *z2 = (size_t *)g_outputs[1], *z3 = (size_t *)g_outputs[2], *z4 = (size_t *)g_outputs[3];
    int32_t *i1 = (int32_t *)g_outputs[0];
    ptrdiff_t *d1 = (ptrdiff_t *)g_outputs[0];
    const uint32_t B = SWH_UNBOUNDED;
    const swh_scope_t s = NULL;
    const swh_levenshtein_t e = NULL;
    const swh_nw_t nw = NULL;
    const swh_sw_t sw = NULL;
    swh_scope_t scope_out = NULL;
    swh_prepared_t prepared_out = NULL;
    swh_levenshtein_t lev_out = NULL;
    swh_nw_t nw_out = NULL;
    swh_sw_t sw_out = NULL;
    swh_sharded_t sharded_out = NULL;
    swh_sharded_cross_t product_out = NULL;
    void *pointer_out = NULL;
    int devices[2] = {0, 0}, device_count = -1;
    int8_t matrix[1] = {0};
    uint8_t classes[1] = {0};
    swh_timing_t timing;
    swh_timing_totals_t totals;
    swh_shard_timing_t shard_timing;
    swh_prepared_info_t info;
    v.tape = NULL; v.first = 0; v.count = 1;
    memset(g_outputs, SENTINEL, sizeof g_outputs);

    /* scopes: creation says that there is no device; everything that takes a scope refuses a null one */
    ND(swh_scope_init_gpu, none, (0, &scope_out, &err));
    ND(swh_scope_init_gpu_stream, none, (0, NULL, &scope_out, &err));
    ND(swh_scope_init_cpu, swh_not_implemented_k, (1, &scope_out, &err));
    ND(swh_scope_init_gpus, none, (devices, 2, &scope_out, &err));
    ND_PLAIN(swh_device_count, fine, (&device_count));
    if (device_count != 0 || scope_out != NULL) report("nodevice.handles", "a device count or a scope handle without a device");
    ND_PLAIN(swh_scope_device_count, bad, (s, z1));
    ND_PLAIN(swh_scope_free, fine, (s));
    ND_PLAIN(swh_scope_compute_units, bad, (s, z1));
    ND_PLAIN(swh_scope_set_async, bad, (s, 1));
    ND(swh_scope_synchronize, bad, (s, &err));
    ND(swh_scope_set_pipelined, bad, (s, 1, &err));
    ND(swh_scope_join, bad, (s, &err));
    ND_PLAIN(swh_scope_forget, bad, (s));
    ND_PLAIN(swh_scope_describe, bad, (s, (char *)g_outputs[0], sizeof g_outputs[0]));
    ND_PLAIN(swh_scope_set_profiling, bad, (s, 1));
    memset(&timing, SENTINEL, sizeof timing); memset(&totals, SENTINEL, sizeof totals); memset(&shard_timing, SENTINEL, sizeof shard_timing);
    memset(&info, SENTINEL, sizeof info);
    ND_PLAIN(swh_scope_last_timing, bad, (s, &timing));
    ND_PLAIN(swh_scope_timing_totals, bad, (s, &totals));
    ND_PLAIN(swh_scope_shard_timing, bad, (s, &shard_timing));
    if (untouched("timing structs", &timing, sizeof timing) || untouched("timing structs", &totals, sizeof totals) ||
        untouched("timing structs", &shard_timing, sizeof shard_timing))
        report("nodevice.timing_structs", g_message);
    /* memory */
    ND(swh_unified_alloc, bad, (s, 64, &pointer_out, &err));
    ND_PLAIN(swh_unified_free, fine, (s, NULL));
    ND(swh_device_alloc, bad, (s, 64, &pointer_out, &err));
    ND_PLAIN(swh_device_free, fine, (s, NULL));
    ND(swh_copy_to_device, bad, (s, g_outputs[0], g_outputs[1], 16, &err));
    ND(swh_copy_to_host, bad, (s, g_outputs[0], g_outputs[1], 16, &err));
    /* prepared tapes */
    ND(swh_tape_prepare_u32, bad, (s, &a32, 0, &prepared_out, &err));
    ND(swh_tape_prepare_u64, bad, (s, &a, 1, &prepared_out, &err));
    ND_PLAIN(swh_prepared_info, bad, (NULL, &info));
    ND_PLAIN(swh_prepared_free, fine, (NULL));
    if (untouched("info", &info, sizeof info)) report("nodevice.prepared_info_struct", g_message);
    /* engines */
    ND(swh_levenshtein_init, bad, (s, 0, 1, 1, 1, &lev_out, &err));
    ND_PLAIN(swh_levenshtein_free, fine, (e));
    ND_PLAIN(swh_levenshtein_set_algorithm, bad, (e, swh_algorithm_tiled_k));
    ND(swh_nw_init, bad, (s, matrix, -4, -4, &nw_out, &err));
    ND(swh_nw_init_classes, bad, (s, classes, matrix, -4, -4, &nw_out, &err));
    ND_PLAIN(swh_nw_free, fine, (nw));
    ND(swh_sw_init, bad, (s, matrix, -4, -4, &sw_out, &err));
    ND(swh_sw_init_classes, bad, (s, classes, matrix, -4, -4, &sw_out, &err));
    ND_PLAIN(swh_sw_free, fine, (sw));
    /* distances and scores */
    ND(swh_levenshtein_pairs_u32tape, bad, (e, s, &a32, &b32, B, o1, 0, &err));
    ND(swh_levenshtein_pairs_u64tape, bad, (e, s, &a, &b, B, o1, 0, &err));
    ND(swh_levenshtein_utf8_pairs_u32tape, bad, (e, s, &a32, &b32, B, o1, 0, &err));
    ND(swh_levenshtein_utf8_pairs_u64tape, bad, (e, s, &a, &b, B, o1, 0, &err));
    ND(swh_levenshtein_cross_u64tape, bad, (e, s, &a, &b, z1, 0, &err));
    ND(swh_levenshtein_utf8_cross_u64tape, bad, (e, s, &a, NULL, z1, 0, &err));
    ND(swh_levenshtein_pairs_prepared, bad, (e, s, &v, &v, B, o1, 0, &err));
    ND(swh_levenshtein_cross_prepared, bad, (e, s, &v, NULL, z1, 0, &err));
    ND(swh_nw_pairs_u32tape, bad, (nw, s, &a32, &b32, i1, 0, &err));
    ND(swh_nw_pairs_u64tape, bad, (nw, s, &a, &b, i1, 0, &err));
    ND(swh_nw_cross_u64tape, bad, (nw, s, &a, &b, d1, 0, &err));
    ND(swh_nw_pairs_prepared, bad, (nw, s, &v, &v, i1, 0, &err));
    ND(swh_nw_cross_prepared, bad, (nw, s, &v, &v, d1, 0, &err));
    ND(swh_sw_pairs_u32tape, bad, (sw, s, &a32, &b32, i1, 0, &err));
    ND(swh_sw_pairs_u64tape, bad, (sw, s, &a, &b, i1, 0, &err));
    ND(swh_sw_cross_u64tape, bad, (sw, s, &a, &b, d1, 0, &err));
    ND(swh_sw_pairs_prepared, bad, (sw, s, &v, &v, i1, 0, &err));
    ND(swh_sw_cross_prepared, bad, (sw, s, &v, &v, d1, 0, &err));
    /* searches and alignments */
    ND(swh_levenshtein_topk_u64tape, bad, (e, s, &a, &b, 2, B, o1, o2, &err));
    ND(swh_levenshtein_utf8_topk_u64tape, bad, (e, s, &a, NULL, 2, B, o1, o2, &err));
    ND(swh_levenshtein_topk_prepared, bad, (e, s, &v, &v, 2, B, o1, o2, &err));
    ND(swh_levenshtein_within_u64tape, bad, (e, s, &a, &b, 2, z4, o1, o2, 8, &err));
    ND(swh_levenshtein_utf8_within_u64tape, bad, (e, s, &a, NULL, 2, z4, o1, o2, 8, &err));
    ND(swh_levenshtein_within_prepared, bad, (e, s, &v, &v, 2, z4, o1, o2, 8, &err));
    ND(swh_levenshtein_align_u64tape, bad, (e, s, &a, &b, B, o1, z4, (char *)o2, 64, &err));
    ND(swh_levenshtein_utf8_align_u64tape, bad, (e, s, &a, &b, B, o1, z4, (char *)o2, 64, &err));
    ND(swh_levenshtein_align_prepared, bad, (e, s, &v, &v, B, o1, z4, (char *)o2, 64, &err));
    /* infix search and the scored families probe for a device on a null handle: swh_no_device_k */
    ND(swh_levenshtein_infix_u64tape, none, (e, s, &a, &b, B, o1, o2, o3, &err));
    ND(swh_levenshtein_utf8_infix_u64tape, none, (e, s, &a, &b, B, o1, o2, o3, &err));
    ND(swh_levenshtein_infix_prepared, none, (e, s, &v, &v, B, o1, o2, o3, &err));
    ND(swh_levenshtein_osa_pairs_u64tape, none, (e, s, &a, &b, B, o1, 0, &err));
    ND(swh_levenshtein_utf8_osa_pairs_u64tape, none, (e, s, &a, &b, B, o1, 0, &err));
    ND(swh_levenshtein_osa_pairs_prepared, none, (e, s, &v, &v, B, o1, 0, &err));
    ND(swh_levenshtein_osa_cross_u64tape, none, (e, s, &a, &b, z1, 0, &err));
    ND(swh_levenshtein_utf8_osa_cross_u64tape, none, (e, s, &a, NULL, z1, 0, &err));
    ND(swh_levenshtein_osa_cross_prepared, none, (e, s, &v, NULL, z1, 0, &err));
    ND(swh_levenshtein_lcs_pairs_u64tape, none, (e, s, &a, &b, B, o1, o2, 0, &err));
    ND(swh_levenshtein_utf8_lcs_pairs_u64tape, none, (e, s, &a, &b, B, o1, o2, 0, &err));
    ND(swh_levenshtein_lcs_pairs_prepared, none, (e, s, &v, &v, B, o1, o2, 0, &err));
    ND(swh_levenshtein_lcs_cross_u64tape, none, (e, s, &a, &b, z1, z2, 0, &err));
    ND(swh_levenshtein_utf8_lcs_cross_u64tape, none, (e, s, &a, NULL, z1, z2, 0, &err));
    ND(swh_levenshtein_lcs_cross_prepared, none, (e, s, &v, NULL, z1, z2, 0, &err));
    ND(swh_levenshtein_jaro_pairs_u64tape, none, (e, s, &a, &b, o1, o2, o3, 0, &err));
    ND(swh_levenshtein_utf8_jaro_pairs_u64tape, none, (e, s, &a, &b, o1, o2, o3, 0, &err));
    ND(swh_levenshtein_jaro_pairs_prepared, none, (e, s, &v, &v, o1, o2, o3, 0, &err));
    ND(swh_levenshtein_jaro_cross_u64tape, none, (e, s, &a, &b, z1, z2, z3, 0, &err));
    ND(swh_levenshtein_utf8_jaro_cross_u64tape, none, (e, s, &a, NULL, z1, z2, z3, 0, &err));
    ND(swh_levenshtein_jaro_cross_prepared, none, (e, s, &v, NULL, z1, z2, z3, 0, &err));
    /* several GPUs behind one scope */
    ND(swh_sharded_prepare_u32tape, bad, (s, &a32, &b32, 0, &sharded_out, &err));
    ND(swh_sharded_prepare_u64tape, bad, (s, &a, &b, 0, &sharded_out, &err));
    ND_PLAIN(swh_sharded_free, fine, (NULL));
    ND_PLAIN(swh_sharded_cuts, bad, (NULL, z1, 4));
    ND(swh_levenshtein_pairs_sharded, bad, (e, s, NULL, B, o1, &err));
    ND(swh_levenshtein_pairs_sharded_u64tape, bad, (e, s, &a, &b, B, o1, &err));
    ND(swh_sharded_cross_prepare_u64tape, bad, (s, &a, &b, 0, &product_out, &err));
    ND_PLAIN(swh_sharded_cross_free, fine, (NULL));
    ND(swh_levenshtein_cross_sharded, bad, (e, s, NULL, z1, 0, &err));
    ND(swh_nw_cross_sharded, bad, (nw, s, NULL, d1, 0, &err));
    ND(swh_sw_cross_sharded, bad, (sw, s, NULL, d1, 0, &err));
    ND(swh_nw_pairs_sharded, bad, (nw, s, NULL, i1, &err));
    ND(swh_sw_pairs_sharded, bad, (sw, s, NULL, i1, &err));
    if (prepared_out || lev_out || nw_out || sw_out || sharded_out || product_out || pointer_out) report("nodevice.handles_out", "a refused call returned a handle");
    /* introspection needs no device */
    report("nodevice.swh_version", swh_version() && *swh_version() ? NULL : "empty");
    report("nodevice.swh_capabilities", swh_capabilities() && *swh_capabilities() ? NULL : "empty");
    free(offsets32);
}

int main(int argc, char **argv) {
    int devices = 0;
    if (argc != 2) die("usage: check_c <case file>", "");
    setvbuf(stdout, NULL, _IOLBF, 0);   /* a line per check, also into a pipe */
    load_case(argv[1]);
    swh_device_count(&devices);
    introspection();
    if (devices == 0) without_a_device();
    else with_a_device();
    free_case();
    fprintf(stderr, "check_c: %d difference%s\n", g_failures, g_failures == 1 ? "" : "s");
    return g_failures ? 1 : 0;
}
