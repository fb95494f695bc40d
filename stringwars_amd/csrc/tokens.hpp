// tokens.hpp -- launchers of the token kernels (tokens.hip), called by two_tape.hip: the token-sorted normal forms of a byte tape's
// strings (swh_tape_token_sort) and the per-pair split of two SWH_TOKENS_UNIQUE tapes into the joined differences X = A - B and
// Y = B - A (swh_levenshtein_token_set_pairs_*).
//
// Neither kernel knows where its results go before it has run: a normal form, X and Y are each never longer than the string they come
// from, so the kernels write them into a staging buffer laid out as the source view is -- string i's result starts where string i
// starts, relative to the view's first byte -- with the lengths beside them. The lengths are scanned into offsets by the offsets
// scan (scan.hpp: launch_offsets_scan) and k_token_compact moves every result to its place in the tape that is kept.
#pragma once
#include "common.hpp"

namespace swh {

// A launch is made for strings of at most kTokenSmallBytes bytes (128 tokens: 1 KB of LDS a wave, every wave slot of a compute unit
// filled) or of at most SWH_TOKEN_MAX_BYTES (2048 tokens: 13 KB, twice that for the split).
constexpr uint32_t kTokenSmallBytes = 256;

// Strings [0, view.count) of a device byte tape with `off64`-wide offsets, whose bytes are [base, base + span) of view.data; `total`
// bytes may be read from view.data at all (the tape's own end: offsets that do not ascend are clamped, not followed).
struct TokenSide {
    TapeRef view;
    uint32_t off64;
    uint64_t base, span, total;
};

struct TokenDerive {
    TokenSide src;
    uint32_t utf8, form;                  // the whitespace set; SWH_TOKENS_SORTED or SWH_TOKENS_UNIQUE
    uint8_t *staging;                     // src.span bytes
    uint32_t *lengths;                    // src.view.count: the bytes of every normal form
    unsigned long long *first_oversize;   // the first string over the launch's limit (atomicMin; ~0 before)
};
void launch_token_derive(Scope *scope, const TokenDerive &d, bool small);

// Pair i is (a[i], b[i]) of two SWH_TOKENS_UNIQUE tapes. x_staging / y_staging (a.span / b.span bytes) and x_lengths / y_lengths
// (bytes) describe X and Y as above; sect, ab and ba (packed u32, any may be null) are the symbols of the joined intersection, of X
// and of Y -- bytes, or with `utf8` the bytes that are no continuation bytes.
struct TokenSplit {
    TokenSide a, b;
    uint32_t utf8;
    uint8_t *x_staging, *y_staging;
    uint32_t *x_lengths, *y_lengths;
    uint32_t *sect, *ab, *ba;
};
void launch_token_set_split(Scope *scope, const TokenSplit &s, bool small);

// Result i, lengths[i] bytes at staging + (offset of string i in `like` - like.base), goes to out + starts[i]; out_offsets[i] = starts[i]
// for i in [0, count] at the width `out_off64` (starts holds count + 1 entries: the scan's row offsets).
struct TokenCompact {
    TokenSide like;
    const uint8_t *staging;
    const uint32_t *lengths;
    const uint64_t *starts;
    uint8_t *out;
    void *out_offsets;
    uint32_t out_off64;
};
void launch_token_compact(Scope *scope, const TokenCompact &c);

}  // namespace swh
