/* check_c_tokens -- the null-handle pass of check_c (check_c.c, `nodevice.<symbol>` lines) for the token scorers' entry points,
 * swh_tape_token_sort, swh_prepared_read and swh_levenshtein_token_set_pairs_*, linked into check_c beside check_c.c as
 * check_c_partial.c is. The five calls are made once, before main() and so before the program touches a device: they get null
 * handles, which no device is needed to refuse -- swh_no_device_k where none is visible, swh_invalid_argument_k where one is; a
 * message is set, the outputs keep their sentinel and no handle is made. What they gave is kept as text; when the program exits the
 * five lines are printed (no library call is made then), one per symbol, `ok` or what differs, and a difference ends the program
 * with status 1. (tests/test_token_ratios.py makes the same calls through ctypes.) */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "stringwars_amd.h"

#define SENTINEL 0xA5

static unsigned char g_outs[4][64];
static char g_lines[5][256];
static int g_line_count = 0, g_differences = 0;

static void line(const char *symbol, int status, int want, const char *error, const char *other) {
    size_t i;
    const char *problem = other;
    char text[160];
    if (status != want) {
        snprintf(text, sizeof text, "status %d, the header documents %d (%s)", status, want, error ? error : "");
        problem = text;
    } else if (!error || !*error) problem = "no error message";
    for (i = 0; i < sizeof g_outs && !problem; ++i)
        if (((const unsigned char *)g_outs)[i] != SENTINEL) problem = "a refused call wrote to its outputs";
    snprintf(g_lines[g_line_count++], sizeof g_lines[0], "nodevice.%s: %s\n", symbol, problem ? problem : "ok");
    if (problem) ++g_differences;
    memset(g_outs, SENTINEL, sizeof g_outs);
}

static void report_at_exit(void) {
    int i;
    for (i = 0; i < g_line_count; ++i) fputs(g_lines[i], stdout);
    fflush(stdout);
    if (g_differences) _exit(1);
}

__attribute__((constructor)) static void tokens_without_handles(void) {
    static const uint64_t offsets[2] = {0, 3};
    static const uint8_t data[3] = {'b', ' ', 'a'};
    const swh_tape_u64_t tape = {data, offsets, 1};
    swh_prepared_view_t view;
    swh_prepared_t derived = (swh_prepared_t)g_outs;   /* (anything but NULL: the refusal clears it) */
    uint32_t *o32[4];
    const char *err = NULL;
    int devices = 0, want, status, k;
    view.tape = NULL; view.first = 0; view.count = 1;
    for (k = 0; k < 4; ++k) o32[k] = (uint32_t *)g_outs[k];
    swh_device_count(&devices);
    want = devices == 0 ? (int)swh_no_device_k : (int)swh_invalid_argument_k;
    memset(g_outs, SENTINEL, sizeof g_outs);
    status = (int)swh_tape_token_sort(NULL, &view, SWH_TOKENS_SORTED, &derived, &err);
    line("swh_tape_token_sort", status, want, err, derived ? "a refused call left a handle" : NULL);
    err = NULL;
    status = (int)swh_prepared_read(NULL, NULL, g_outs[0], (size_t *)g_outs[1], &err);
    line("swh_prepared_read", status, want, err, NULL);
    err = NULL;
    status = (int)swh_levenshtein_token_set_pairs_u64tape(NULL, NULL, &tape, &tape, o32[0], o32[1], o32[2], o32[3], 0, &err);
    line("swh_levenshtein_token_set_pairs_u64tape", status, want, err, NULL);
    err = NULL;
    status = (int)swh_levenshtein_utf8_token_set_pairs_u64tape(NULL, NULL, &tape, &tape, o32[0], o32[1], o32[2], o32[3], 4, &err);
    line("swh_levenshtein_utf8_token_set_pairs_u64tape", status, want, err, NULL);
    err = NULL;
    status = (int)swh_levenshtein_token_set_pairs_prepared(NULL, NULL, &view, &view, o32[0], NULL, o32[2], NULL, 0, &err);
    line("swh_levenshtein_token_set_pairs_prepared", status, want, err, NULL);
    atexit(report_at_exit);
}
