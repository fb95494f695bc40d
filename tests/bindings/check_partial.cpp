// check_partial -- the C++ wrappers of the partial ratio (LevenshteinDistances::partial and ::partial_cross of
// include/stringwars_amd.hpp, the raw and the prepared overload of each) called as a user's program calls them. Built and driven by
// tests/test_partial_ratio.py, which compares what this program writes with its references.
//
//   check_partial <case file> <result file>
//
// Case file (little-endian, no padding): i32 utf8; u64 count, the count + 1 u64 offsets of tape a, its bytes; the same for tape b (as
// many strings). Result file: four calls, each the arrays lcs, starts, ends, sides --
//   partial on the raw tapes (count u32 each), partial on the prepared tapes (count u32 each),
//   partial_cross a x b on the raw tapes (count x count u64 each), partial_cross a x a on the prepared tape (count x count u64 each).
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

template <typename T> struct Outputs {
    std::vector<T> lcs, starts, ends, sides;
    explicit Outputs(size_t n) : lcs(n, (T)77), starts(n, (T)77), ends(n, (T)77), sides(n, (T)77) {}
    swa::LevenshteinDistances::PartialCounts<T> counts() { return {lcs.data(), starts.data(), ends.data(), sides.data()}; }
    void write(std::FILE *out) const {
        for (const std::vector<T> *v : {&lcs, &starts, &ends, &sides}) std::fwrite(v->data(), sizeof(T), v->size(), out);
    }
};

template <typename Engine>
void run(std::FILE *out, const Tape &ta, const Tape &tb, bool utf8) {
    const swa::DeviceScope scope = swa::DeviceScope::gpu_device(0);
    const Engine engine(scope);
    const swa::BytesTapeView a = ta.view(), b = tb.view();
    const swa::PreparedTape pa(scope, a, utf8), pb(scope, b, utf8);
    Outputs<uint32_t> raw(a.count), prepared(a.count);
    engine.partial(scope, raw.counts(), a, b);
    raw.write(out);
    engine.partial(scope, prepared.counts(), pa, pb);
    prepared.write(out);
    Outputs<size_t> cross(a.count * b.count), own(a.count * a.count);
    engine.partial_cross(scope, cross.counts(), a, &b);
    cross.write(out);
    engine.partial_cross(scope, own.counts(), pa, nullptr);
    own.write(out);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: check_partial <case file> <result file>\n"); return 3; }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "check_partial: cannot open the files\n"); return 3; }
    int status = 0;
    try {
        const bool utf8 = take<int32_t>(in) != 0;
        const Tape a = take_tape(in), b = take_tape(in);
        if (a.offsets.size() != b.offsets.size()) throw std::runtime_error("the two tapes hold different numbers of strings");
        if (utf8) run<swa::LevenshteinDistancesUtf8>(out, a, b, true);
        else run<swa::LevenshteinDistances>(out, a, b, false);
    } catch (const swa::Error &e) {
        std::fprintf(stderr, "check_partial: status %d: %s\n", (int)e.status, e.what());
        status = 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "check_partial: %s\n", e.what());
        status = 2;
    }
    std::fclose(in);
    std::fclose(out);
    return status;
}
