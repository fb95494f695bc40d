// check_infix_all -- the C++ wrappers of the infix search for every occurrence (LevenshteinDistances::infix_all of
// include/stringwars_amd.hpp, both overloads) called as a user's program calls them: a counting call, then a filled call with
// exactly the room the first one counted. Built and driven by tests/test_infix_all.py, which compares what this program writes with
// its reference exactly.
//
//   check_infix_all <case file> <result file>
//
// Case file (little-endian, no padding): i32 utf8; u64 count, the count + 1 u64 offsets of the patterns, their bytes; the same for
// the texts; u32 request count; per request i32 prepared (the PreparedTape overload), i32 with_starts, u32 bound, u32 select.
// Result file: per request the count + 1 u64 row offsets of the counting call, those of the filled call, then the u32 starts (only
// with_starts), ends and distances. Exit status 0 when every call returned; a thrown error is printed and ends with 2.
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
void run(std::FILE *in, std::FILE *out, const Tape &patterns, const Tape &texts, bool utf8) {
    using Out = typename Engine::InfixOccurrencesOut;
    const swa::DeviceScope scope = swa::DeviceScope::gpu_device(0);
    const Engine engine(scope);
    const swa::BytesTapeView p = patterns.view(), t = texts.view();
    const swa::PreparedTape pp(scope, p, utf8), pt(scope, t, utf8);
    const uint32_t requests = take<uint32_t>(in);
    for (uint32_t r = 0; r < requests; ++r) {
        const int prepared = take<int32_t>(in), with_starts = take<int32_t>(in);
        const uint32_t bound = take<uint32_t>(in), select = take<uint32_t>(in);
        std::vector<size_t> counted(p.count + 1, 0xA5A5A5A5u), offsets(p.count + 1, 0xA5A5A5A5u);
        std::vector<uint32_t> starts, ends, distances;
        for (int filled = 0; filled < 2; ++filled) {
            Out o;
            o.row_offsets = (filled ? offsets : counted).data();
            if (filled) {
                for (std::vector<uint32_t> *array : {&starts, &ends, &distances}) array->assign(counted[p.count] + 1, 0xA5A5A5A5u);   // (+ 1: never empty)
                o.starts = with_starts ? starts.data() : nullptr;
                o.ends = ends.data();
                o.distances = distances.data();
                o.capacity = counted[p.count];
            }
            if (prepared) engine.infix_all(scope, o, pp, pt, bound, select);
            else engine.infix_all(scope, o, p, t, bound, select);
        }
        static_assert(sizeof(size_t) == 8, "row offsets are written as 64-bit words");
        std::fwrite(counted.data(), 8, counted.size(), out);
        std::fwrite(offsets.data(), 8, offsets.size(), out);
        if (with_starts) std::fwrite(starts.data(), 4, offsets[p.count], out);
        std::fwrite(ends.data(), 4, offsets[p.count], out);
        std::fwrite(distances.data(), 4, offsets[p.count], out);
        const size_t spare = counted[p.count];
        if (starts[spare] != 0xA5A5A5A5u || ends[spare] != 0xA5A5A5A5u || distances[spare] != 0xA5A5A5A5u) throw std::runtime_error("written past the capacity");
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: check_infix_all <case file> <result file>\n"); return 3; }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "check_infix_all: cannot open the files\n"); return 3; }
    int status = 0;
    try {
        const bool utf8 = take<int32_t>(in) != 0;
        const Tape patterns = take_tape(in), texts = take_tape(in);
        if (utf8) run<swa::LevenshteinDistancesUtf8>(in, out, patterns, texts, true);
        else run<swa::LevenshteinDistances>(in, out, patterns, texts, false);
    } catch (const swa::Error &e) {
        std::fprintf(stderr, "check_infix_all: status %d: %s\n", (int)e.status, e.what());
        status = 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "check_infix_all: %s\n", e.what());
        status = 2;
    }
    std::fclose(in);
    std::fclose(out);
    return status;
}
