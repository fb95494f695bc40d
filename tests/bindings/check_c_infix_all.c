/* check_c_infix_all -- the null-handle pass of check_c (check_c.c, `nodevice.<symbol>` lines) for the entry points of the infix search
 * for every occurrence, swh_levenshtein_infix_all_*, linked into check_c beside check_c.c as check_c_extract_within.c is. The three
 * calls are made once, before main() and so before the program touches a device: they get null handles, which no device is needed to
 * refuse -- swh_no_device_k where none is visible, swh_invalid_argument_k where one is; a message is set, and the four outputs keep
 * their sentinel. What they gave is kept as text; when the program exits the three lines are printed (no library call is made then),
 * one per symbol, `ok` or what differs, and a difference ends the program with status 1. (tests/test_infix_all.py makes the same
 * calls through ctypes.) */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "stringwars_amd.h"

#define SENTINEL 0xA5

static unsigned char g_offsets[64], g_starts[64], g_ends[64], g_distances[64];
static char g_lines[3][256];
static int g_line_count = 0, g_differences = 0;

static void fill_sentinels(void) {
    memset(g_offsets, SENTINEL, sizeof g_offsets);
    memset(g_starts, SENTINEL, sizeof g_starts);
    memset(g_ends, SENTINEL, sizeof g_ends);
    memset(g_distances, SENTINEL, sizeof g_distances);
}

static void line(const char *symbol, int status, int want, const char *error) {
    size_t i;
    const char *problem = NULL;
    char text[160];
    if (status != want) {
        snprintf(text, sizeof text, "status %d, the header documents %d (%s)", status, want, error ? error : "");
        problem = text;
    } else if (!error || !*error) problem = "no error message";
    for (i = 0; i < sizeof g_ends && !problem; ++i)
        if (g_offsets[i] != SENTINEL || g_starts[i] != SENTINEL || g_ends[i] != SENTINEL || g_distances[i] != SENTINEL)
            problem = "a refused call wrote to its outputs";
    snprintf(g_lines[g_line_count++], sizeof g_lines[0], "nodevice.%s: %s\n", symbol, problem ? problem : "ok");
    if (problem) ++g_differences;
    fill_sentinels();
}

static void report_at_exit(void) {
    int i;
    for (i = 0; i < g_line_count; ++i) fputs(g_lines[i], stdout);
    fflush(stdout);
    if (g_differences) _exit(1);
}

__attribute__((constructor)) static void infix_all_without_handles(void) {
    static const uint64_t offsets[2] = {0, 1};
    static const uint8_t data[1] = {'a'};
    const swh_tape_u64_t tape = {data, offsets, 1};
    swh_prepared_view_t view;
    const char *err = NULL;
    int devices = 0, want, status;
    view.tape = NULL; view.first = 0; view.count = 1;
    swh_device_count(&devices);
    want = devices == 0 ? (int)swh_no_device_k : (int)swh_invalid_argument_k;
    fill_sentinels();
    err = NULL;
    status = (int)swh_levenshtein_infix_all_u64tape(NULL, NULL, &tape, &tape, 1, SWH_INFIX_SELECT_ALL, (size_t *)g_offsets, (uint32_t *)g_starts,
                                                    (uint32_t *)g_ends, (uint32_t *)g_distances, 4, &err);
    line("swh_levenshtein_infix_all_u64tape", status, want, err);
    err = NULL;
    status = (int)swh_levenshtein_utf8_infix_all_u64tape(NULL, NULL, &tape, &tape, SWH_UNBOUNDED, SWH_INFIX_SELECT_BEST, (size_t *)g_offsets,
                                                         (uint32_t *)g_starts, (uint32_t *)g_ends, (uint32_t *)g_distances, 4, &err);
    line("swh_levenshtein_utf8_infix_all_u64tape", status, want, err);
    err = NULL;
    status = (int)swh_levenshtein_infix_all_prepared(NULL, NULL, &view, &view, 0, SWH_INFIX_SELECT_MINIMA, (size_t *)g_offsets,
                                                     (uint32_t *)g_starts, (uint32_t *)g_ends, (uint32_t *)g_distances, 4, &err);
    line("swh_levenshtein_infix_all_prepared", status, want, err);
    atexit(report_at_exit);
}
