// check_extract_within -- the C++ wrappers of the score range search (LevenshteinDistances::extract_within of
// include/stringwars_amd.hpp, both overloads) called as a user's program calls them: a counting call, then a filled call with
// exactly the room the first one counted. Built and driven by tests/test_extract_within.py, which compares what this program writes
// with its references bit for bit.
//
//   check_extract_within <case file> <result file>
//
// Case file (little-endian, no padding): i32 utf8; u64 nq, the nq + 1 u64 offsets of the queries, their bytes; the same for the
// candidates; u32 request count; per request i32 scorer, i32 prepared (the PreparedTape overload), i32 self (no candidates: the
// queries against themselves), f64 cutoff, f64 prefix weight. Result file: per request the nq + 1 u64 row offsets of the counting
// call, those of the filled call, the u32 indices and the doubles. Exit status 0 when every call returned; a thrown error is printed
// and ends with 2.
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
        const double cutoff = take<double>(in), prefix_weight = take<double>(in);
        std::vector<size_t> counted(q.count + 1, 0xA5A5A5A5u), offsets(q.count + 1, 0xA5A5A5A5u);
        std::vector<uint32_t> indices;
        std::vector<double> scores;
        for (int filled = 0; filled < 2; ++filled) {
            std::vector<size_t> &rows = filled ? offsets : counted;
            if (filled) { indices.assign(counted[q.count] + 1, 0xA5A5A5A5u); scores.assign(counted[q.count] + 1, -7.0); }   // (+ 1: never empty)
            uint32_t *ind = filled ? indices.data() : nullptr;
            double *sco = filled ? scores.data() : nullptr;
            const size_t capacity = filled ? counted[q.count] : 0;
            if (prepared) engine.extract_within(scope, scorer, pq, self ? nullptr : &pc, cutoff, rows.data(), ind, sco, capacity, prefix_weight);
            else engine.extract_within(scope, scorer, q, self ? nullptr : &c, cutoff, rows.data(), ind, sco, capacity, prefix_weight);
        }
        static_assert(sizeof(size_t) == 8, "row offsets are written as 64-bit words");
        std::fwrite(counted.data(), 8, counted.size(), out);
        std::fwrite(offsets.data(), 8, offsets.size(), out);
        std::fwrite(indices.data(), 4, offsets[q.count], out);
        std::fwrite(scores.data(), 8, offsets[q.count], out);
        if (indices[counted[q.count]] != 0xA5A5A5A5u || scores[counted[q.count]] != -7.0) throw std::runtime_error("written past the capacity");
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: check_extract_within <case file> <result file>\n"); return 3; }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "check_extract_within: cannot open the files\n"); return 3; }
    int status = 0;
    try {
        const bool utf8 = take<int32_t>(in) != 0;
        const Tape queries = take_tape(in), candidates = take_tape(in);
        if (utf8) run<swa::LevenshteinDistancesUtf8>(in, out, queries, candidates, true);
        else run<swa::LevenshteinDistances>(in, out, queries, candidates, false);
    } catch (const swa::Error &e) {
        std::fprintf(stderr, "check_extract_within: status %d: %s\n", (int)e.status, e.what());
        status = 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "check_extract_within: %s\n", e.what());
        status = 2;
    }
    std::fclose(in);
    std::fclose(out);
    return status;
}
