// check_tokens -- the C++ wrappers of the token scorers (PreparedTape::token_sorted and ::read, LevenshteinDistances::token_set on raw
// and on prepared tapes, token_set_score of include/stringwars_amd.hpp) called as a user's program calls them. Built and driven by
// tests/test_token_ratios.py, which compares what this program writes with its references.
//
//   check_tokens <case file> <result file>
//
// Case file (little-endian, no padding): i32 utf8; u64 count, the count + 1 u64 offsets of tape a, its bytes; the same for tape b (as
// many strings). Result file, in this order:
//   the SWH_TOKENS_SORTED tape of a, then of b, then the SWH_TOKENS_UNIQUE tape of a: each count + 1 u64 offsets and the bytes;
//   indel and lcs of the two sorted tapes (count u32 each): token_sort_ratio is their ratio;
//   sect, ab, ba, lcs of token_set on the raw tapes (count u32 each), then of token_set on the two unique tapes (derived here);
//   token_set_score of the raw call's counts (count f64).
// Exit status 0 when every call returned; a thrown error is printed and ends with 2.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "stringwars_amd.hpp"

namespace {

template <typename T> T take(std::FILE *in) {
    T value{};
    if (std::fread(&value, sizeof value, 1, in) != 1) throw std::runtime_error("short case file");
    return value;
}

struct Tape {
    std::vector<uint64_t> offsets;
    std::vector<uint8_t> data;
    swa::BytesTapeView view() const { return swa::BytesTapeView{data.data(), offsets.data(), offsets.size() - 1}; }
};

Tape take_tape(std::FILE *in) {
    Tape tape;
    const uint64_t count = take<uint64_t>(in);
    tape.offsets.resize(count + 1);
    if (std::fread(tape.offsets.data(), 8, count + 1, in) != count + 1) throw std::runtime_error("short case file");
    tape.data.resize(tape.offsets.back() + 1);   // (one spare byte: data() of an empty tape stays a pointer)
    if (tape.offsets.back() && std::fread(tape.data.data(), 1, tape.offsets.back(), in) != tape.offsets.back()) throw std::runtime_error("short case file");
    return tape;
}

void write_tape(std::FILE *out, const swa::DeviceScope &scope, const swa::PreparedTape &tape) {
    std::vector<size_t> offsets;
    const std::vector<uint8_t> data = tape.read(scope, offsets);
    static_assert(sizeof(size_t) == 8, "the offsets are written as u64");
    std::fwrite(offsets.data(), 8, offsets.size(), out);
    std::fwrite(data.data(), 1, data.size(), out);
}

struct Outputs {
    std::vector<uint32_t> sect, ab, ba, lcs;
    explicit Outputs(size_t n) : sect(n, 77u), ab(n, 77u), ba(n, 77u), lcs(n, 77u) {}
    swa::LevenshteinDistances::TokenSetCounts<uint32_t> counts() { return {sect.data(), ab.data(), ba.data(), lcs.data()}; }
    void write(std::FILE *out) const {
        for (const std::vector<uint32_t> *v : {&sect, &ab, &ba, &lcs}) std::fwrite(v->data(), 4, v->size(), out);
    }
};

template <typename Engine>
void run(std::FILE *out, const Tape &ta, const Tape &tb, bool utf8) {
    const swa::DeviceScope scope = swa::DeviceScope::gpu_device(0);
    const Engine engine(scope);
    const swa::BytesTapeView a = ta.view(), b = tb.view();
    const swa::PreparedTape pa(scope, a, utf8), pb(scope, b, utf8);
    const swa::PreparedTape sorted_a = pa.token_sorted(scope), sorted_b = pb.token_sorted(scope, SWH_TOKENS_SORTED);
    const swa::PreparedTape unique_a = pa.token_sorted(scope, SWH_TOKENS_UNIQUE), unique_b = pb.token_sorted(scope, SWH_TOKENS_UNIQUE);
    write_tape(out, scope, sorted_a);
    write_tape(out, scope, sorted_b);
    write_tape(out, scope, unique_a);
    std::vector<uint32_t> indel(a.count, 77u), lcs(a.count, 77u);
    engine.lcs(scope, sorted_a, sorted_b, indel.data(), lcs.data());
    std::fwrite(indel.data(), 4, indel.size(), out);
    std::fwrite(lcs.data(), 4, lcs.size(), out);
    Outputs raw(a.count), prepared(a.count);
    engine.token_set(scope, raw.counts(), a, b);
    raw.write(out);
    engine.token_set(scope, prepared.counts(), unique_a, unique_b);
    prepared.write(out);
    std::vector<double> scores(a.count);
    for (size_t i = 0; i < a.count; ++i) scores[i] = swa::token_set_score(raw.sect[i], raw.ab[i], raw.ba[i], raw.lcs[i]);
    std::fwrite(scores.data(), 8, scores.size(), out);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: check_tokens <case file> <result file>\n"); return 3; }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "check_tokens: cannot open the files\n"); return 3; }
    int status = 0;
    try {
        const bool utf8 = take<int32_t>(in) != 0;
        const Tape a = take_tape(in), b = take_tape(in);
        if (a.offsets.size() != b.offsets.size()) throw std::runtime_error("the two tapes hold different numbers of strings");
        if (utf8) run<swa::LevenshteinDistancesUtf8>(out, a, b, true);
        else run<swa::LevenshteinDistances>(out, a, b, false);
    } catch (const swa::Error &e) {
        std::fprintf(stderr, "check_tokens: status %d: %s\n", (int)e.status, e.what());
        status = 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "check_tokens: %s\n", e.what());
        status = 2;
    }
    std::fclose(in);
    std::fclose(out);
    return status;
}
