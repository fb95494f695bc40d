// topk_fold.hpp -- the rank merge of the searches that keep k results per row (topk.hip, extract.hip), with the key as a type
// parameter. A row's running list is its k smallest keys so far, sorted, padded with the key type's pad; a wave's 64 fresh keys are
// admitted with one compare against the wave-uniform threshold and one ballot, and the admitted ones are merged here.
//
// What a key type brings is its KeyOps: `pad()` (above every real key), `less(a, b)` (a strict total order in which real keys are
// distinct) and `readlane(key, lane)`.
//   uint64_t   topk.hip's (d << 32) | j
//   WideKey    extract.hip's (64-bit score pattern, 32-bit candidate index), compared lexicographically
#pragma once
#include "cross_words.hpp"

namespace swh {

template <typename Key> struct KeyOps;

template <> struct KeyOps<uint64_t> {
    static __device__ __forceinline__ uint64_t pad() { return ~0ull; }
    static __device__ __forceinline__ bool less(uint64_t a, uint64_t b) { return a < b; }
    static __device__ __forceinline__ uint64_t readlane(uint64_t v, int lane) { return readlane64(v, lane); }
};

// The key of a search that ranks by a float64 score: the score's bit pattern (complemented where the larger score is the better one:
// non-negative doubles order as their patterns do) and the candidate index. Nothing narrower would do: two scores that differ as
// doubles may agree in their upper 32 bits.
struct WideKey {
    uint64_t score;
    uint32_t index;
};
template <> struct KeyOps<WideKey> {
    static __device__ __forceinline__ WideKey pad() { return WideKey{~0ull, 0xFFFFFFFFu}; }
    static __device__ __forceinline__ bool less(const WideKey &a, const WideKey &b) {
        return a.score < b.score || (a.score == b.score && a.index < b.index);
    }
    static __device__ __forceinline__ WideKey readlane(const WideKey &v, int lane) {
        return WideKey{readlane64(v.score, lane), (uint32_t)__builtin_amdgcn_readlane((int)v.index, lane)};
    }
};

// Merges the keys of the `admitted` lanes into the wave's sorted list of k keys (LDS, k <= 64) and returns the new threshold.
// Keys are distinct (candidate indices are), and no admitted key is a pad: ranks in the union are a permutation. A key's place in
// the new list is the number of list entries below it plus the number of admitted keys below it, every list entry moves down by
// the admitted keys below it, and whatever lands at k or beyond drops out.
template <typename Key>
__device__ __forceinline__ Key topk_fold(Key *list, uint32_t k, Key key, uint64_t admitted, Key cap) {
    using Ops = KeyOps<Key>;
    const uint32_t lane = __lane_id();
    const Key own = lane < k ? list[lane] : Ops::pad();
    uint32_t below_key = 0, below_own = 0;
    for (uint64_t rest = admitted; rest; rest &= rest - 1) {
        const Key other = Ops::readlane(key, __builtin_ctzll(rest));
        below_key += Ops::less(other, key) ? 1u : 0u;
        below_own += Ops::less(other, own) ? 1u : 0u;
    }
    uint32_t at = 0;   // list entries below my key
#pragma unroll
    for (uint32_t step = 64; step; step >>= 1)
        if (at + step <= k && Ops::less(list[at + step - 1], key)) at += step;
    lds_order();
    if ((admitted >> lane) & 1ull) {
        const uint32_t rank = at + below_key;
        if (rank < k) list[rank] = key;
    }
    if (lane < k) {
        const uint32_t rank = lane + below_own;
        if (rank < k) list[rank] = own;
    }
    lds_order();
    const Key last = list[k - 1];
    return Ops::less(last, cap) ? last : cap;
}

}  // namespace swh
