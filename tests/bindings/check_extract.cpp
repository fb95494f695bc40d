// check_extract -- the C++ wrappers of the score search (LevenshteinDistances::extract of include/stringwars_amd.hpp, both overloads)
// called as a user's program calls them. Built and driven by tests/test_extract.py, which compares what this program writes with its
// references bit for bit.
//
//   check_extract <case file> <result file>
//
// Case file (little-endian, no padding): i32 utf8; u64 nq, the nq + 1 u64 offsets of the queries, their bytes; the same for the
// candidates; u32 request count; per request i32 scorer, i32 prepared (the PreparedTape overload), i32 self (no candidates: the
// queries against themselves), u64 k, f64 cutoff (NaN: `no_cutoff(scorer)`), f64 prefix weight. Result file: per request the
// nq x k u32 indices, then the nq x k doubles. Exit status 0 when every call returned; a thrown error is printed and ends with 2.
#include <cmath>
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

template <typename Engine>
void run(std::FILE *in, std::FILE *out, const Tape &queries, const Tape &candidates, bool utf8) {
    const swa::DeviceScope scope = swa::DeviceScope::gpu_device(0);
    const Engine engine(scope);
    const swa::BytesTapeView q = queries.view(), c = candidates.view();
    const swa::PreparedTape pq(scope, q, utf8), pc(scope, c, utf8);
    const uint32_t requests = take<uint32_t>(in);
    for (uint32_t r = 0; r < requests; ++r) {
        const int scorer = take<int32_t>(in), prepared = take<int32_t>(in), self = take<int32_t>(in);
        const uint64_t k = take<uint64_t>(in);
        double cutoff = take<double>(in);
        const double prefix_weight = take<double>(in);
        if (std::isnan(cutoff)) cutoff = swa::LevenshteinDistances::no_cutoff(scorer);
        std::vector<uint32_t> indices(q.count * k, 0xA5A5A5A5u);
        std::vector<double> scores(q.count * k, -7.0);
        if (prepared) engine.extract(scope, scorer, pq, self ? nullptr : &pc, k, indices.data(), scores.data(), cutoff, prefix_weight);
        else engine.extract(scope, scorer, q, self ? nullptr : &c, k, indices.data(), scores.data(), cutoff, prefix_weight);
        std::fwrite(indices.data(), 4, indices.size(), out);
        std::fwrite(scores.data(), 8, scores.size(), out);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: check_extract <case file> <result file>\n"); return 3; }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "check_extract: cannot open the files\n"); return 3; }
    int status = 0;
    try {
        const bool utf8 = take<int32_t>(in) != 0;
        const Tape queries = take_tape(in), candidates = take_tape(in);
        if (utf8) run<swa::LevenshteinDistancesUtf8>(in, out, queries, candidates, true);
        else run<swa::LevenshteinDistances>(in, out, queries, candidates, false);
    } catch (const swa::Error &e) {
        std::fprintf(stderr, "check_extract: status %d: %s\n", (int)e.status, e.what());
        status = 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "check_extract: %s\n", e.what());
        status = 2;
    }
    std::fclose(in);
    std::fclose(out);
    return status;
}
