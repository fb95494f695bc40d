// tokens.hip -- the token kernels: the token-sorted normal forms of a tape's strings (swh_tape_token_sort; rapidfuzz
// fuzz.token_sort_ratio is fuzz.ratio of two of them) and the split of two sorted unique token lists into what they share and what
// each has alone (swh_levenshtein_token_set_pairs_*; fuzz.token_set_ratio). include/stringwars_amd.h states the contract: tokens are
// the maximal runs of non-whitespace symbols (Python's split()), ordered bytewise with a proper prefix first (Python's sorted(); on
// valid UTF-8 byte order is code-point order, so both modes compare bytes), joined by one 0x20.
//
// One wave (a workgroup of 64 lanes) works on one string, which it holds in LDS whole: at most SWH_TOKEN_MAX_BYTES bytes and, beside
// them, a table of at most half as many tokens as packed words, start << 16 | length.
//  - Whitespace is flagged per byte from the staged string, a 64-bit __ballot per 64 bytes. A multi-byte UTF-8 space is recognised at
//    its lead byte from the next one or two bytes and at its other bytes from the one or two before: all reads are of the LDS copy,
//    which is padded with zeros, so a sequence that lies across two 64-byte steps is read like any other.
//  - A token starts at a byte that is no whitespace and whose predecessor is (or is the string's start): the __ballot of that, and a
//    token's slot in the table is the popcount of the mask below its lane. It ends at the next flagged byte, found in the masks.
//  - Up to 64 tokens are ranked, one per lane (n comparisons a lane); more run a bitonic network over the next power of two in LDS
//    (log^2 steps: 2048 tokens are 66 steps of 16 compare-exchanges a lane). The order is made total by the start offset, so the
//    keys are distinct and every run gives the same table.
//  - SWH_TOKENS_UNIQUE drops a token that equals its predecessor in sorted order. A kept token goes to the exclusive prefix sum of
//    length + 1 over the kept ones (a wave scan per 64 tokens), the separator in front of it: no atomics, the same bytes every run.
// Where the results lie -- tokens.hpp -- is decided after the kernel: it writes into staging laid out like its source.
#include <algorithm>

#include "tokens.hpp"

namespace swh {

constexpr uint32_t kTokenPad = 0xFFFFFFFFu;   // an entry of the sorting network past the last token: after every token
constexpr uint32_t kTokenLaneCopy = 32;       // a token of at most this many bytes is copied by its own lane, a longer one by the wave
constexpr uint64_t kTokenMostBlocks = 1u << 22;

__device__ __forceinline__ uint64_t token_offset(const TokenSide &s, uint64_t i) {
    return s.off64 ? ((const uint64_t *)s.view.offsets)[i] : (uint64_t)((const uint32_t *)s.view.offsets)[i];
}
// String i of a side: where it starts behind the side's first byte, and its bytes -- none where the offsets do not ascend or point
// outside [base, base + span) or the tape.
__device__ __forceinline__ void token_extent(const TokenSide &s, uint64_t i, uint64_t &rel, uint64_t &len) {
    const uint64_t s0 = token_offset(s, i), s1 = token_offset(s, i + 1);
    rel = 0; len = 0;
    if (s0 < s.base || s1 < s0) return;
    const uint64_t r = s0 - s.base, l = s1 - s0;
    if (r > s.span || l > s.span - r || s0 > s.total || l > s.total - s0) return;
    rel = r; len = l;
}

// What a wave holds of one string of at most MAXB bytes.
template <int MAXB> struct TokenString {
    uint64_t ws[MAXB / 64];     // bit p % 64 of word p / 64: byte p is whitespace, or lies past the end
    uint32_t tab[MAXB / 2];     // the tokens: start << 16 | length
    uint8_t str[MAXB + 8];      // the bytes, zeros behind them
};

template <int MAXB> __device__ __forceinline__ void token_stage(TokenString<MAXB> &s, const uint8_t *src, uint32_t len) {
    for (uint32_t p = threadIdx.x; p < len + 3; p += 64) s.str[p] = p < len ? src[p] : (uint8_t)0;
}

// bytes.split(): 09 0A 0B 0C 0D 20
struct WsBytes {
    __device__ __forceinline__ bool operator()(const uint8_t *s, uint32_t p) const { return s[p] == 0x20 || (s[p] >= 0x09 && s[p] <= 0x0D); }
};
// the separator of a normal form
struct WsSpace {
    __device__ __forceinline__ bool operator()(const uint8_t *s, uint32_t p) const { return s[p] == 0x20; }
};
// str.isspace(), in UTF-8: U+0009-000D, U+001C-0020, U+0085, U+00A0, U+1680, U+2000-200A, U+2028, U+2029, U+202F, U+205F, U+3000
struct WsUtf8 {
    // the bytes of the whitespace sequence that starts at p, 0 where none does
    static __device__ __forceinline__ uint32_t sequence(const uint8_t *s, uint32_t p) {
        const uint32_t b0 = s[p], b1 = s[p + 1], b2 = s[p + 2];
        if ((b0 >= 0x09 && b0 <= 0x0D) || (b0 >= 0x1C && b0 <= 0x20)) return 1;
        if (b0 == 0xC2) return b1 == 0x85 || b1 == 0xA0 ? 2 : 0;
        if (b0 == 0xE1) return b1 == 0x9A && b2 == 0x80 ? 3 : 0;
        if (b0 == 0xE2) {
            if (b1 == 0x80) return (b2 >= 0x80 && b2 <= 0x8A) || b2 == 0xA8 || b2 == 0xA9 || b2 == 0xAF ? 3 : 0;
            return b1 == 0x81 && b2 == 0x9F ? 3 : 0;
        }
        if (b0 == 0xE3) return b1 == 0x80 && b2 == 0x80 ? 3 : 0;
        return 0;
    }
    __device__ __forceinline__ bool operator()(const uint8_t *s, uint32_t p) const {
        return sequence(s, p) >= 1 || (p >= 1 && sequence(s, p - 1) >= 2) || (p >= 2 && sequence(s, p - 2) >= 3);
    }
};

// Flags the staged string's whitespace and lists its tokens in s.tab, in the order they stand; returns how many. Ends on a barrier.
template <int MAXB, typename Ws> __device__ uint32_t token_table(TokenString<MAXB> &s, uint32_t len, Ws is_ws) {
    const uint32_t lane = threadIdx.x, words = (len + 63) >> 6;
    for (uint32_t w = 0; w < words; ++w) {
        const uint32_t p = w * 64 + lane;
        const uint64_t mask = __ballot(p >= len || is_ws(s.str, p));
        if (lane == 0) s.ws[w] = mask;
    }
    __syncthreads();
    uint32_t count = 0;
    for (uint32_t w = 0; w < words; ++w) {
        const uint32_t p = w * 64 + lane;
        const uint64_t word = s.ws[w];
        const bool me = (word >> lane) & 1;
        const bool before = p == 0 || (lane ? (word >> (lane - 1)) & 1 : s.ws[w - 1] >> 63);
        const bool start = !me && before;
        const uint64_t starts = __ballot(start);
        if (start) {
            uint32_t end = len;
            const uint64_t rest = word >> lane;
            if (rest) {
                end = p + (uint32_t)__builtin_ctzll(rest);
            } else {
                for (uint32_t v = w + 1; v < words; ++v) {
                    if (s.ws[v]) { end = v * 64 + (uint32_t)__builtin_ctzll(s.ws[v]); break; }
                }
            }
            s.tab[count + __popcll(starts & ((1ull << lane) - 1))] = p << 16 | (end - p);
        }
        count += __popcll(starts);
    }
    __syncthreads();
    return count;
}

// bytewise, a proper prefix first: < 0, 0, > 0
__device__ __forceinline__ int token_cmp(const uint8_t *sx, uint32_t x, const uint8_t *sy, uint32_t y) {
    const uint32_t lx = x & 0xFFFF, ly = y & 0xFFFF, n = lx < ly ? lx : ly;
    const uint8_t *px = sx + (x >> 16), *py = sy + (y >> 16);
    for (uint32_t k = 0; k < n; ++k) {
        const int d = (int)px[k] - (int)py[k];
        if (d) return d;
    }
    return (int)lx - (int)ly;
}
// the sorting order of one string's table: equal tokens by where they start (the high half of the word)
__device__ __forceinline__ bool token_less(const uint8_t *s, uint32_t x, uint32_t y) {
    if (x == kTokenPad || y == kTokenPad) return x != kTokenPad;
    const int c = token_cmp(s, x, s, y);
    return c < 0 || (c == 0 && x < y);
}

// Sorts s.tab[0, count). Begins after a barrier and ends on one.
template <int MAXB> __device__ void token_sort(TokenString<MAXB> &s, uint32_t count) {
    const uint32_t lane = threadIdx.x;
    if (count <= 64) {   // a token per lane: its rank is the number of tokens before it
        const uint32_t mine = lane < count ? s.tab[lane] : kTokenPad;
        uint32_t rank = 0;
        if (lane < count)
            for (uint32_t j = 0; j < count; ++j) rank += token_less(s.str, s.tab[j], mine) ? 1u : 0u;
        __syncthreads();
        if (lane < count) s.tab[rank] = mine;
        __syncthreads();
        return;
    }
    uint32_t n = 128;
    while (n < count) n <<= 1;   // (at most MAXB / 2, a power of two)
    for (uint32_t j = count + lane; j < n; j += 64) s.tab[j] = kTokenPad;
    __syncthreads();
    for (uint32_t k = 2; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j; j >>= 1) {
            for (uint32_t t = lane; t < n / 2; t += 64) {   // the t-th compare-exchange of the step: entries lo and lo + j
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const bool ascending = (lo & k) == 0;
                const uint32_t x = s.tab[lo], y = s.tab[hi];
                if (token_less(s.str, y, x) == ascending) { s.tab[lo] = y; s.tab[hi] = x; }
            }
            __syncthreads();
        }
    }
}

// Joins the tokens j of tab[0, count) that keep(j, tab[j]) names, in table order, with one 0x20 between them: into `out` (or nowhere:
// null). `bytes`: the length of the join; `continuation`, with `count_continuation`: how many of its bytes are UTF-8 continuation bytes.
template <typename Keep>
__device__ void token_emit(const uint8_t *str, const uint32_t *tab, uint32_t count, Keep keep, uint8_t *out, bool count_continuation,
                           uint32_t &bytes, uint32_t &continuation) {
    const uint32_t lane = threadIdx.x;
    const bool touch = out || count_continuation;
    uint32_t total = 0, cont = 0;
    for (uint32_t j0 = 0; j0 < count; j0 += 64) {
        const uint32_t j = j0 + lane;
        const uint32_t e = j < count ? tab[j] : 0u;
        const bool kept = j < count && keep(j, e);
        const uint32_t length = e & 0xFFFF, start = e >> 16, room = kept ? length + 1 : 0u;
        uint32_t upto = room;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t below = __shfl_up(upto, d);
            if (lane >= (uint32_t)d) upto += below;
        }
        const uint32_t dest = total + upto - room;
        total += __shfl(upto, 63);
        if (kept && out && dest) out[dest - 1] = 0x20;
        if (kept && touch && length <= kTokenLaneCopy) {
            for (uint32_t q = 0; q < length; ++q) {
                const uint8_t b = str[start + q];
                if (out) out[dest + q] = b;
                cont += (b & 0xC0) == 0x80 ? 1u : 0u;
            }
        }
        uint64_t longs = touch ? __ballot(kept && length > kTokenLaneCopy) : 0ull;
        while (longs) {   // (the same mask in every lane)
            const int from = __builtin_ctzll(longs);
            longs &= longs - 1;
            const uint32_t e_from = __shfl(e, from), dest_from = __shfl(dest, from);
            for (uint32_t q = lane; q < (e_from & 0xFFFF); q += 64) {
                const uint8_t b = str[(e_from >> 16) + q];
                if (out) out[dest_from + q] = b;
                cont += (b & 0xC0) == 0x80 ? 1u : 0u;
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) cont += __shfl_xor(cont, d);
    bytes = total ? total - 1 : 0u;
    continuation = count_continuation ? cont : 0u;
}

template <int MAXB> __global__ void __launch_bounds__(64) k_token_derive(TokenDerive d) {
    __shared__ TokenString<MAXB> s;
    const bool unique = d.form == SWH_TOKENS_UNIQUE;
    for (uint64_t i = blockIdx.x; i < d.src.view.count; i += gridDim.x) {
        uint64_t rel, len64;
        token_extent(d.src, i, rel, len64);
        if (len64 > MAXB) {   // (the whole wave: the call fails, or runs again for longer strings)
            if (threadIdx.x == 0) { atomicMin(d.first_oversize, (unsigned long long)i); d.lengths[i] = 0; }
            continue;
        }
        const uint32_t len = (uint32_t)len64;
        token_stage(s, (const uint8_t *)d.src.view.data + d.src.base + rel, len);
        __syncthreads();
        const uint32_t count = d.utf8 ? token_table(s, len, WsUtf8{}) : token_table(s, len, WsBytes{});
        token_sort(s, count);
        uint32_t bytes, continuation;
        token_emit(s.str, s.tab, count,
                   [&](uint32_t j, uint32_t e) { return !unique || j == 0 || token_cmp(s.str, s.tab[j - 1], s.str, e) != 0; },
                   d.staging + rel, false, bytes, continuation);
        if (threadIdx.x == 0) d.lengths[i] = bytes;
        __syncthreads();   // the next string's staging overwrites what the lanes still read
    }
}

// is token x (of string sx) one of the sorted distinct tokens tab[0, count) of string sy
__device__ __forceinline__ bool token_find(const uint8_t *sx, uint32_t x, const uint8_t *sy, const uint32_t *tab, uint32_t count) {
    uint32_t lo = 0, hi = count;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const int c = token_cmp(sx, x, sy, tab[mid]);
        if (c == 0) return true;
        if (c < 0) hi = mid; else lo = mid + 1;
    }
    return false;
}

template <int MAXB> struct TokenPair {
    TokenString<MAXB> a, b;
    uint64_t a_in_b[MAXB / 128], b_in_a[MAXB / 128];   // bit j % 64 of word j / 64: token j of the side is a token of the other
};

// Both sides are normal forms, so their tables, cut at the single spaces, are sorted and distinct as they stand: membership is a
// binary search, and what is kept of a side comes out in sorted order.
template <int MAXB> __global__ void __launch_bounds__(64) k_token_set_split(TokenSplit t) {
    __shared__ TokenPair<MAXB> s;
    const uint32_t lane = threadIdx.x;
    const bool utf8 = t.utf8 != 0;
    for (uint64_t i = blockIdx.x; i < t.a.view.count; i += gridDim.x) {
        uint64_t rel_a, la64, rel_b, lb64;
        token_extent(t.a, i, rel_a, la64);
        token_extent(t.b, i, rel_b, lb64);
        if (la64 > MAXB || lb64 > MAXB) la64 = lb64 = 0;   // (no tape this library derived holds such a string: the pair counts nothing)
        const uint32_t la = (uint32_t)la64, lb = (uint32_t)lb64;
        token_stage(s.a, (const uint8_t *)t.a.view.data + t.a.base + rel_a, la);
        token_stage(s.b, (const uint8_t *)t.b.view.data + t.b.base + rel_b, lb);
        __syncthreads();
        const uint32_t na = token_table(s.a, la, WsSpace{}), nb = token_table(s.b, lb, WsSpace{});
        for (uint32_t j0 = 0; j0 < na; j0 += 64) {
            const uint32_t j = j0 + lane;
            const uint64_t found = __ballot(j < na && token_find(s.a.str, s.a.tab[j < na ? j : 0], s.b.str, s.b.tab, nb));
            if (lane == 0) s.a_in_b[j0 >> 6] = found;
        }
        for (uint32_t j0 = 0; j0 < nb; j0 += 64) {
            const uint32_t j = j0 + lane;
            const uint64_t found = __ballot(j < nb && token_find(s.b.str, s.b.tab[j < nb ? j : 0], s.a.str, s.a.tab, na));
            if (lane == 0) s.b_in_a[j0 >> 6] = found;
        }
        __syncthreads();
        uint32_t x_bytes, x_cont, y_bytes, y_cont, s_bytes, s_cont;
        token_emit(s.a.str, s.a.tab, na, [&](uint32_t j, uint32_t) { return !((s.a_in_b[j >> 6] >> (j & 63)) & 1); }, t.x_staging + rel_a, utf8,
                   x_bytes, x_cont);
        token_emit(s.b.str, s.b.tab, nb, [&](uint32_t j, uint32_t) { return !((s.b_in_a[j >> 6] >> (j & 63)) & 1); }, t.y_staging + rel_b, utf8,
                   y_bytes, y_cont);
        token_emit(s.a.str, s.a.tab, na, [&](uint32_t j, uint32_t) { return (bool)((s.a_in_b[j >> 6] >> (j & 63)) & 1); }, (uint8_t *)nullptr, utf8,
                   s_bytes, s_cont);
        if (lane == 0) {
            t.x_lengths[i] = x_bytes;
            t.y_lengths[i] = y_bytes;
            if (t.sect) t.sect[i] = s_bytes - s_cont;
            if (t.ab) t.ab[i] = x_bytes - x_cont;
            if (t.ba) t.ba[i] = y_bytes - y_cont;
        }
        __syncthreads();
    }
}

// A wave per result; wave count, the one past the last, writes the closing offset alone.
__global__ void __launch_bounds__(256) k_token_compact(TokenCompact c) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t count = c.like.view.count, waves = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i <= count; i += waves) {
        const uint64_t at = c.starts[i];
        if (lane == 0) {
            if (c.out_off64) ((uint64_t *)c.out_offsets)[i] = at;
            else ((uint32_t *)c.out_offsets)[i] = (uint32_t)at;
        }
        if (i == count) break;
        uint64_t rel, len;
        token_extent(c.like, i, rel, len);
        const uint64_t n = std::min<uint64_t>(c.lengths[i], len);
        for (uint64_t q = lane; q < n; q += 64) c.out[at + q] = c.staging[rel + q];
    }
}

static uint32_t token_blocks(uint64_t strings) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(strings, kTokenMostBlocks)); }

void launch_token_derive(Scope *scope, const TokenDerive &d, bool small) {
    StampGuard guard(scope, "token_derive");
    if (small) hipLaunchKernelGGL(k_token_derive<(int)kTokenSmallBytes>, dim3(token_blocks(d.src.view.count)), dim3(64), 0, scope->stream, d);
    else hipLaunchKernelGGL(k_token_derive<(int)SWH_TOKEN_MAX_BYTES>, dim3(token_blocks(d.src.view.count)), dim3(64), 0, scope->stream, d);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_token_set_split(Scope *scope, const TokenSplit &s, bool small) {
    StampGuard guard(scope, "token_set_split");
    if (small) hipLaunchKernelGGL(k_token_set_split<(int)kTokenSmallBytes>, dim3(token_blocks(s.a.view.count)), dim3(64), 0, scope->stream, s);
    else hipLaunchKernelGGL(k_token_set_split<(int)SWH_TOKEN_MAX_BYTES>, dim3(token_blocks(s.a.view.count)), dim3(64), 0, scope->stream, s);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_token_compact(Scope *scope, const TokenCompact &c) {
    StampGuard guard(scope, "token_compact");
    const uint64_t blocks = (c.like.view.count + 1 + 3) / 4;
    hipLaunchKernelGGL(k_token_compact, dim3(token_blocks(blocks)), dim3(256), 0, scope->stream, c);
    SWH_HIP_CHECK(hipGetLastError());
}

}  // namespace swh
