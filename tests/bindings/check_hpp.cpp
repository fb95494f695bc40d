// check_hpp -- every engine wrapper of include/stringwars_amd.hpp, called as a C++ user calls it, against expected arrays.
//
//   check_hpp <case file>
//
// The case file is written by tests/test_bindings.py from the suite's references. Format (little-endian, no padding): the 8 bytes
// "SWCASE1\0", a u32 array count, then per array a u32 name length, the name, a u32 dtype code (0 u8, 1 u32, 2 u64, 3 i32, 4 i64,
// 5 i8), a u64 element count and the elements. Array names are listed where they are read.
//
// One line per method and variant on stdout: `<Class>.<method>[<form>|<variant>]: ok`, or the first difference. Every output array is
// filled with the sentinel byte 0xA5 before the call and carries one more element than the call may write: an element that still
// holds the sentinel, a padding byte between two rows or the element past the end that does not, is a difference. Exit status 0 when
// every line is ok. With no device visible only the constructors run: each must throw swa::Error with the documented status.
#include <cinttypes>
#include <map>

#include "stringwars_amd.hpp"

namespace {

constexpr uint8_t kSentinel = 0xA5;
constexpr size_t kWidth[6] = {1, 4, 8, 4, 8, 1};

struct Array { uint32_t dtype = 0; uint64_t count = 0; std::vector<uint8_t> bytes; };
std::map<std::string, Array> g_case;
int g_failures = 0;

[[noreturn]] void die(const std::string &what) {
    std::fprintf(stderr, "check_hpp: %s\n", what.c_str());
    std::exit(3);
}

void load_case(const char *path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) die(std::string("cannot open ") + path);
    char magic[8];
    uint32_t arrays = 0;
    in.read(magic, 8);
    in.read((char *)&arrays, 4);
    if (!in || std::memcmp(magic, "SWCASE1\0", 8) != 0) die("not a case file");
    for (uint32_t i = 0; i < arrays; ++i) {
        uint32_t length = 0;
        in.read((char *)&length, 4);
        std::string name(length, ' ');
        in.read(&name[0], length);
        Array a;
        in.read((char *)&a.dtype, 4);
        in.read((char *)&a.count, 8);
        if (!in || a.dtype > 5) die("bad array header");
        a.bytes.resize(a.count * kWidth[a.dtype] + 8);   // (+ 8: never a null data())
        in.read((char *)a.bytes.data(), (std::streamsize)(a.count * kWidth[a.dtype]));
        if (!in) die("short case file at " + name);
        g_case[name] = std::move(a);
    }
}

template <typename T> const T *arr(const std::string &name, size_t *count = nullptr) {
    auto it = g_case.find(name);
    if (it == g_case.end()) die("the case file has no array " + name);
    if (kWidth[it->second.dtype] != sizeof(T)) die("array " + name + " has another element width");
    if (count) *count = (size_t)it->second.count;
    return (const T *)it->second.bytes.data();
}

swa::BytesTapeView tape(const std::string &name) {
    size_t entries = 0;
    const uint64_t *offsets = arr<uint64_t>(name + ".off", &entries);
    return swa::BytesTapeView{arr<uint8_t>(name + ".data"), offsets, entries - 1};
}

/// rows x cols elements of `elem` bytes, rows `stride` bytes apart, then a guard as large again (a wrapper that passed twice the
/// stride still writes inside the buffer, where it is seen); all sentinel.
struct Out {
    std::vector<uint8_t> bytes;
    size_t elem, rows, cols, stride;
    Out(size_t elem_, size_t rows_, size_t cols_, size_t stride_bytes = 0)
        : elem(elem_), rows(rows_), cols(cols_), stride(stride_bytes ? stride_bytes : cols_ * elem_) {
        bytes.assign(2 * rows * stride + elem + 64, kSentinel);
    }
    template <typename T> T *as() { return (T *)bytes.data(); }
    uint64_t value(size_t row, size_t col) const {
        uint64_t v = 0;
        std::memcpy(&v, bytes.data() + row * stride + col * elem, elem);
        return v;
    }
};

std::string untouched(const Out &o, const char *what) {
    for (size_t i = 0; i < o.bytes.size(); ++i)
        if (o.bytes[i] != kSentinel) return std::string(what) + ": written at byte " + std::to_string(i) + ", must stay at its sentinel";
    return "";
}

/// "" when `o` holds want[row * want_ld + col] everywhere, its padding and its guard are untouched; else the first difference.
template <typename T> std::string diff(const Out &o, const T *want, size_t want_ld, const char *what) {
    char text[160];
    for (size_t r = 0; r < o.rows; ++r) {
        for (size_t c = 0; c < o.cols; ++c) {
            uint64_t w = 0;
            std::memcpy(&w, &want[r * want_ld + c], sizeof(T));
            if (o.value(r, c) != w) {
                uint64_t untouched_value = 0;
                std::memset(&untouched_value, kSentinel, sizeof(T));
                if (o.value(r, c) == untouched_value)
                    std::snprintf(text, sizeof text, "%s: the sentinel survived at index %zu (row %zu, column %zu): want %" PRIu64, what, r * o.cols + c, r, c, w);
                else
                std::snprintf(text, sizeof text, "%s: first difference at index %zu (row %zu, column %zu): got %" PRIu64 " want %" PRIu64, what,
                              r * o.cols + c, r, c, o.value(r, c), w);
                return text;
            }
        }
        for (size_t b = r * o.stride + o.cols * o.elem; b < (r + 1) * o.stride; ++b)
            if (o.bytes[b] != kSentinel) {
                std::snprintf(text, sizeof text, "%s: padding byte %zu of row %zu was written", what, b - r * o.stride, r);
                return text;
            }
    }
    for (size_t b = o.rows * o.stride; b < o.bytes.size(); ++b)
        if (o.bytes[b] != kSentinel) {
            std::snprintf(text, sizeof text, "%s: byte %zu past the end was written", what, b - o.rows * o.stride);
            return text;
        }
    return "";
}

std::string first_of(std::initializer_list<std::string> problems) {
    for (const std::string &p : problems)
        if (!p.empty()) return p;
    return "";
}

template <typename Body> void run(const std::string &name, Body body) {
    std::string problem;
    try {
        problem = body();
    } catch (const swa::Error &e) {
        problem = "swa::Error status " + std::to_string((int)e.status) + ": " + e.what();
    }
    std::printf("%s: %s\n", name.c_str(), problem.empty() ? "ok" : problem.c_str());
    if (!problem.empty()) ++g_failures;
}

uint32_t g_pair_bound = 0, g_search_bound = 0;

// ---- the pairwise wrappers: pairs_into, osa, lcs, jaro, infix, align on pairs [lo, hi) of <P>.pa / <P>.pb -----------------------------------
// expected: <P>.lev, .osa, .indel (+ _b: at the bound), .lcs, .jaro_m / _t / _p, .infix_d / _s / _e (+ _b), .align_off / .align_ops (+ _b)
template <typename T>
void pairwise(const std::string &cls, const std::string &form, const swa::LevenshteinDistances &engine, const swa::DeviceScope &scope, const T &a,
              const T &b, const std::string &P, size_t lo, size_t hi) {
    const size_t n = hi - lo;
    auto name = [&](const char *method, const std::string &variant) { return cls + "." + method + "[" + form + "|" + variant + "]"; };
    auto want = [&](const char *key) { return arr<uint32_t>(P + "." + key) + lo; };
    for (int bounded = 0; bounded < 2; ++bounded) {
        const uint32_t bound = bounded ? g_pair_bound : SWH_UNBOUNDED;
        const std::string tag = bounded ? "bound" : "unbounded";
        run(name("pairs_into", tag), [&] {
            Out out(4, 1, n);
            engine.pairs_into(scope, a, b, out.as<uint32_t>(), bound);
            return diff(out, want(bounded ? "lev_b" : "lev"), 0, "distances");
        });
        run(name("osa", tag), [&] {
            Out out(4, 1, n);
            engine.osa(scope, a, b, out.as<uint32_t>(), bound);
            return diff(out, want(bounded ? "osa_b" : "osa"), 0, "distances");
        });
        for (int which = 0; which < 3; ++which)   // both, indel alone, lcs alone
            run(name("lcs", std::string(which == 0 ? "both" : which == 1 ? "indel" : "lcs") + "|" + tag), [&] {
                Out indel(4, 1, n), lcs(4, 1, n);
                engine.lcs(scope, a, b, which != 2 ? indel.as<uint32_t>() : nullptr, which != 1 ? lcs.as<uint32_t>() : nullptr, bound);
                return first_of({which != 2 ? diff(indel, want(bounded ? "indel_b" : "indel"), 0, "indel") : untouched(indel, "indel"),
                                 which != 1 ? diff(lcs, want("lcs"), 0, "lcs") : untouched(lcs, "lcs")});
            });
        run(name("infix", tag), [&] {
            Out distances(4, 1, n), starts(4, 1, n), ends(4, 1, n);
            engine.infix(scope, a, b, distances.as<uint32_t>(), starts.as<uint32_t>(), ends.as<uint32_t>(), bound);
            return first_of({diff(distances, want(bounded ? "infix_d_b" : "infix_d"), 0, "distances"),
                             diff(starts, want(bounded ? "infix_s_b" : "infix_s"), 0, "starts"), diff(ends, want(bounded ? "infix_e_b" : "infix_e"), 0, "ends")});
        });
        run(name("align", tag), [&] {
            const uint64_t *all_offsets = arr<uint64_t>(P + (bounded ? ".align_off_b" : ".align_off"));
            const uint8_t *all_ops = arr<uint8_t>(P + (bounded ? ".align_ops_b" : ".align_ops"));
            const size_t capacity = (size_t)arr<uint64_t>(P + ".ops_capacity")[0], total = (size_t)(all_offsets[hi] - all_offsets[lo]);
            std::vector<uint64_t> offsets(n + 1);
            for (size_t i = 0; i <= n; ++i) offsets[i] = all_offsets[lo + i] - all_offsets[lo];
            std::vector<uint8_t> ops(capacity, kSentinel);   // the script, then the sentinel: the call writes `total` operations and no more
            std::memcpy(ops.data(), all_ops + all_offsets[lo], total);
            Out distances(4, 1, n), got_offsets(8, 1, n + 1), got_ops(1, 1, capacity);
            engine.align(scope, a, b, distances.as<uint32_t>(), got_offsets.as<size_t>(), got_ops.as<char>(), capacity, bound);
            return first_of({diff(distances, want(bounded ? "lev_b" : "lev"), 0, "distances"), diff(got_offsets, offsets.data(), 0, "ops_offsets"),
                             diff(got_ops, ops.data(), 0, "ops")});
        });
    }
    static const char *const kJaro[4] = {"all", "matches", "transpositions", "prefix"};
    for (int which = 0; which < 4; ++which)
        run(name("jaro", kJaro[which]), [&] {
            Out m(4, 1, n), t(4, 1, n), p(4, 1, n);
            const bool wm = which == 0 || which == 1, wt = which == 0 || which == 2, wp = which == 0 || which == 3;
            engine.jaro(scope, a, b, wm ? m.as<uint32_t>() : nullptr, wt ? t.as<uint32_t>() : nullptr, wp ? p.as<uint32_t>() : nullptr);
            return first_of({wm ? diff(m, want("jaro_m"), 0, "matches") : untouched(m, "matches"),
                             wt ? diff(t, want("jaro_t"), 0, "transpositions") : untouched(t, "transpositions"),
                             wp ? diff(p, want("jaro_p"), 0, "prefix") : untouched(p, "prefix")});
        });
}

// ---- the two-tape wrappers: compute_into, osa_cross, lcs_cross, jaro_cross, topk, within -----------------------------------------------------
// A product: `nq` queries x `nc` candidates (cand == nullptr: the queries themselves). Its dense matrices are the block at (row0, col0)
// of <P>.<dense>.{lev,osa,indel,lcs,jaro_m,jaro_t,jaro_p} (u64, `ld` columns); its searches are <P>.<search>.topk.k<k>.<u|b>.<i|d> and
// <P>.<search>.within.{off,i,d}.
struct Product { const char *tag, *dense, *search; size_t nq, nc, row0, col0, ld; };

template <typename T>
void two_tapes(const std::string &cls, const std::string &form, const swa::LevenshteinDistances &engine, const swa::DeviceScope &scope, const T &q,
               const T *cand, const std::string &P, const Product &x) {
    auto name = [&](const char *method, const std::string &variant) { return cls + "." + method + "[" + form + "|" + variant + "]"; };
    auto want = [&](const char *key) { return arr<uint64_t>(P + "." + x.dense + "." + key) + x.row0 * x.ld + x.col0; };
    for (int padded = 0; padded < 2; ++padded) {
        const size_t stride = padded ? x.nc * 8 + 24 : 0;   // a row and three more elements
        const std::string shape = std::string(x.tag) + "|" + (padded ? "stride" : "packed");
        run(name("compute_into", shape), [&] {
            Out out(8, x.nq, x.nc, stride);
            engine.compute_into(scope, q, cand, out.as<size_t>(), stride);
            return diff(out, want("lev"), x.ld, "matrix");
        });
        run(name("osa_cross", shape), [&] {
            Out out(8, x.nq, x.nc, stride);
            engine.osa_cross(scope, q, cand, out.as<size_t>(), stride);
            return diff(out, want("osa"), x.ld, "matrix");
        });
        for (int which = 0; which < 3; ++which)
            run(name("lcs_cross", std::string(which == 0 ? "both" : which == 1 ? "indel" : "lcs") + "|" + shape), [&] {
                Out indel(8, x.nq, x.nc, stride), lcs(8, x.nq, x.nc, stride);
                engine.lcs_cross(scope, q, cand, which != 2 ? indel.as<size_t>() : nullptr, which != 1 ? lcs.as<size_t>() : nullptr, stride);
                return first_of({which != 2 ? diff(indel, want("indel"), x.ld, "indel") : untouched(indel, "indel"),
                                 which != 1 ? diff(lcs, want("lcs"), x.ld, "lcs") : untouched(lcs, "lcs")});
            });
        static const char *const kJaro[4] = {"all", "matches", "transpositions", "prefix"};
        for (int which = 0; which < 4; ++which)
            run(name("jaro_cross", std::string(kJaro[which]) + "|" + shape), [&] {
                Out m(8, x.nq, x.nc, stride), t(8, x.nq, x.nc, stride), p(8, x.nq, x.nc, stride);
                const bool wm = which == 0 || which == 1, wt = which == 0 || which == 2, wp = which == 0 || which == 3;
                engine.jaro_cross(scope, q, cand, wm ? m.as<size_t>() : nullptr, wt ? t.as<size_t>() : nullptr, wp ? p.as<size_t>() : nullptr, stride);
                return first_of({wm ? diff(m, want("jaro_m"), x.ld, "matches") : untouched(m, "matches"),
                                 wt ? diff(t, want("jaro_t"), x.ld, "transpositions") : untouched(t, "transpositions"),
                                 wp ? diff(p, want("jaro_p"), x.ld, "prefix") : untouched(p, "prefix")});
            });
    }
    const std::string search = P + "." + x.search;
    for (size_t k : {(size_t)1, (size_t)5, (size_t)64})
        for (int bounded = 0; bounded < 2; ++bounded)
            run(name("topk", std::string(x.tag) + "|k" + std::to_string(k) + "|" + (bounded ? "bound" : "unbounded")), [&] {
                const std::string rows = search + ".topk.k" + std::to_string(k) + (bounded ? ".b" : ".u");
                Out indices(4, x.nq, k), distances(4, x.nq, k);
                engine.topk(scope, q, cand, k, indices.as<uint32_t>(), distances.as<uint32_t>(), bounded ? g_search_bound : SWH_UNBOUNDED);
                return first_of({diff(distances, arr<uint32_t>(rows + ".d"), k, "distances"), diff(indices, arr<uint32_t>(rows + ".i"), k, "indices")});
            });
    const uint64_t *offsets = arr<uint64_t>(search + ".within.off");
    const uint32_t *hit_indices = arr<uint32_t>(search + ".within.i"), *hit_distances = arr<uint32_t>(search + ".within.d");
    const size_t total = (size_t)offsets[x.nq];
    run(name("within", std::string(x.tag) + "|count"), [&] {
        Out got(8, 1, x.nq + 1);
        engine.within(scope, q, cand, g_search_bound, got.as<size_t>(), nullptr, nullptr, 0);
        return diff(got, offsets, 0, "row_offsets");
    });
    run(name("within", std::string(x.tag) + "|exact"), [&] {
        Out got(8, 1, x.nq + 1), indices(4, 1, total), distances(4, 1, total);
        engine.within(scope, q, cand, g_search_bound, got.as<size_t>(), indices.as<uint32_t>(), distances.as<uint32_t>(), total);
        return first_of({diff(got, offsets, 0, "row_offsets"), diff(indices, hit_indices, 0, "indices"), diff(distances, hit_distances, 0, "distances")});
    });
    run(name("within", std::string(x.tag) + "|short"), [&] {   // one entry too few: the offsets are written, the arrays are not
        Out got(8, 1, x.nq + 1), indices(4, 1, total - 1), distances(4, 1, total - 1);
        engine.within(scope, q, cand, g_search_bound, got.as<size_t>(), indices.as<uint32_t>(), distances.as<uint32_t>(), total - 1);
        return first_of({diff(got, offsets, 0, "row_offsets"), untouched(indices, "indices"), untouched(distances, "distances")});
    });
}

// Every Levenshtein wrapper in its three forms: raw tapes, prepared tapes, and subviews of the prepared tapes (lo > 0, hi < size). The
// views come and go around uses of their owners: a view that freed or kept its owner's handle shows in what runs next.
template <typename Engine> void levenshtein(const std::string &cls, const swa::DeviceScope &scope, const std::string &P, bool utf8) {
    Engine engine(scope);
    const uint64_t *views = arr<uint64_t>("views");   // pairs lo, hi; queries lo, hi; candidates lo, hi
    const swa::BytesTapeView a = tape(P + ".pa"), b = tape(P + ".pb"), q = tape(P + ".q"), c = tape(P + ".c");
    const Product cross{"candidates", "x", "x", q.count, c.count, 0, 0, c.count}, self{"self", "s", "s", q.count, q.count, 0, 0, q.count};
    const size_t ql = (size_t)views[2], qh = (size_t)views[3], cl = (size_t)views[4], ch = (size_t)views[5];
    const Product view_cross{"candidates", "x", "vx", qh - ql, ch - cl, ql, cl, c.count}, view_self{"self", "s", "vs", qh - ql, qh - ql, ql, ql, q.count};

    pairwise(cls, "raw", engine, scope, a, b, P, 0, a.count);
    two_tapes(cls, "raw", engine, scope, q, &c, P, cross);
    two_tapes<swa::BytesTapeView>(cls, "raw", engine, scope, q, nullptr, P, self);

    swa::PreparedTape pa(scope, a, utf8), pb(scope, b, utf8), pq(scope, q, utf8), pc(scope, c, utf8);
    {
        swa::PreparedTape va = pa.subview((size_t)views[0], (size_t)views[1]), vb = pb.subview((size_t)views[0], (size_t)views[1]);
        pairwise(cls, "subview", engine, scope, va, vb, P, (size_t)views[0], (size_t)views[1]);
        swa::PreparedTape vq = pq.subview(ql, qh), vc = pc.subview(cl, ch);
        two_tapes(cls, "subview", engine, scope, vq, &vc, P, view_cross);
        two_tapes<swa::PreparedTape>(cls, "subview", engine, scope, vq, nullptr, P, view_self);
    }   // the views are gone; their owners must still be whole
    pairwise(cls, "prepared", engine, scope, pa, pb, P, 0, a.count);
    two_tapes(cls, "prepared", engine, scope, pq, &pc, P, cross);
    two_tapes<swa::PreparedTape>(cls, "prepared", engine, scope, pq, nullptr, P, self);
    {   // a view of a view, made after its owner was used and dropped before the owner is used again
        swa::PreparedTape outer = pa.subview(2, a.count - 1), outer_b = pb.subview(2, a.count - 1);
        swa::PreparedTape inner = outer.subview(3, outer.size() - 2), inner_b = outer_b.subview(3, outer_b.size() - 2);
        run(cls + ".subview[nested]", [&] {
            Out out(4, 1, inner.size());
            engine.pairs_into(scope, inner, inner_b, out.as<uint32_t>());
            return first_of({inner.size() == a.count - 8 ? "" : "size() of a nested view", diff(out, arr<uint32_t>(P + ".lev") + 5, 0, "distances")});
        });
    }
    run(cls + ".subview[owner-after-views]", [&] {
        Out out(4, 1, a.count);
        engine.pairs_into(scope, pa, pb, out.as<uint32_t>());
        return first_of({pa.info().count == a.count ? "" : "info().count of the owner", diff(out, arr<uint32_t>(P + ".lev"), 0, "distances")});
    });
}

// ---- NeedlemanWunschScores / SmithWatermanScores: both constructors, both gap models ------------------------------------------------------------
// tapes nw.pa / nw.pb (pairs) and nw.q / nw.c (products); nw.classes (u8[256]), nw.costs (i8[32 x 32]), nw.matrix (i8[256 x 256]);
// expected <nw|sw>.<classes|matrix>.<linear|affine>.<pairs (i32) | cross (i64) | self (i64)>
template <typename Engine> void alignment_engine(const std::string &cls, const std::string &prefix, const swa::DeviceScope &scope, const Engine &engine,
                                                 const std::string &variant) {
    const swa::BytesTapeView a = tape("nw.pa"), b = tape("nw.pb"), q = tape("nw.q"), c = tape("nw.c");
    const std::string expected = prefix + "." + variant + ".";
    std::string label = variant;
    std::replace(label.begin(), label.end(), '.', '|');
    run(cls + ".pairs_into[raw|" + label + "]", [&] {
        Out out(4, 1, a.count);
        engine.pairs_into(scope, a, b, out.as<int32_t>());
        return diff(out, arr<int32_t>(expected + "pairs"), 0, "scores");
    });
    for (int self = 0; self < 2; ++self)
        for (int padded = 0; padded < 2; ++padded)
            run(cls + ".compute_into[raw|" + label + "|" + (self ? "self" : "candidates") + "|" + (padded ? "stride" : "packed") + "]", [&] {
                const size_t nc = self ? q.count : c.count, stride = padded ? nc * 8 + 24 : 0;
                Out out(8, q.count, nc, stride);
                engine.compute_into(scope, q, self ? nullptr : &c, out.as<ptrdiff_t>(), stride);
                return diff(out, arr<int64_t>(expected + (self ? "self" : "cross")), nc, "matrix");
            });
}

template <typename Engine> void alignment(const std::string &cls, const std::string &prefix, const swa::DeviceScope &scope) {
    uint8_t classes[256];
    int8_t costs[32][32];
    std::memcpy(classes, arr<uint8_t>("nw.classes"), sizeof classes);
    std::memcpy(costs, arr<int8_t>("nw.costs"), sizeof costs);
    const int8_t *matrix = arr<int8_t>("nw.matrix");
    const struct { const char *name; int open, extend; } gaps[2] = {{"linear", -4, -4}, {"affine", -11, -1}};
    for (const auto &g : gaps) {
        alignment_engine(cls, prefix, scope, Engine(scope, classes, costs, g.open, g.extend), std::string("classes.") + g.name);
        alignment_engine(cls, prefix, scope, Engine(scope, matrix, g.open, g.extend), std::string("matrix.") + g.name);
    }
}

// ---- no device: every constructor throws the documented status with a message --------------------------------------------------------------------
template <typename Make> void must_throw(const std::string &name, swh_status_t status, Make make) {
    std::string problem = "no swa::Error was thrown";
    try {
        make();
    } catch (const swa::Error &e) {
        problem = e.status != status ? "status " + std::to_string((int)e.status) + ", the header documents " + std::to_string((int)status)
                                     : std::strlen(e.what()) == 0 ? "empty message" : "";
    }
    std::printf("nodevice.%s: %s\n", name.c_str(), problem.empty() ? "ok" : problem.c_str());
    if (!problem.empty()) ++g_failures;
}

void without_a_device() {
    const swa::BytesTapeView bad = tape("bad.a"), other = tape("bad.b");
    uint8_t classes[256] = {0};
    int8_t costs[32][32] = {{0}};
    std::vector<int8_t> matrix(65536, 0);
    swa::DeviceScope none;   // what a caller is left with: no handle
    must_throw("DeviceScope.gpu_device", swh_no_device_k, [] { swa::DeviceScope::gpu_device(0); });
    must_throw("DeviceScope.gpu_devices", swh_no_device_k, [] { swa::DeviceScope::gpu_devices({0, 0}); });
    must_throw("DeviceScope.cpu_cores", swh_not_implemented_k, [] { swa::DeviceScope::cpu_cores(1); });
    must_throw("PreparedTape", swh_invalid_argument_k, [&] { swa::PreparedTape t(none, bad, true); });
    must_throw("LevenshteinDistances", swh_invalid_argument_k, [&] { swa::LevenshteinDistances e(none); });
    must_throw("LevenshteinDistancesUtf8", swh_invalid_argument_k, [&] { swa::LevenshteinDistancesUtf8 e(none); });
    must_throw("NeedlemanWunschScores.classes", swh_invalid_argument_k, [&] { swa::NeedlemanWunschScores e(none, classes, costs, -4, -4); });
    must_throw("NeedlemanWunschScores.matrix", swh_invalid_argument_k, [&] { swa::NeedlemanWunschScores e(none, matrix.data(), -4, -4); });
    must_throw("SmithWatermanScores.classes", swh_invalid_argument_k, [&] { swa::SmithWatermanScores e(none, classes, costs, -4, -4); });
    must_throw("SmithWatermanScores.matrix", swh_invalid_argument_k, [&] { swa::SmithWatermanScores e(none, matrix.data(), -4, -4); });
    must_throw("ShardedPairs", swh_invalid_argument_k, [&] { swa::ShardedPairs s(none, bad, other); });
    must_throw("ShardedCross", swh_invalid_argument_k, [&] { swa::ShardedCross s(none, bad, other); });
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) die("usage: check_hpp <case file>");
    std::setvbuf(stdout, nullptr, _IOLBF, 0);   // a line per check, also into a pipe
    load_case(argv[1]);
    if (swa::DeviceScope::visible_devices() == 0) {
        without_a_device();
        return g_failures ? 1 : 0;
    }
    try {
        g_pair_bound = arr<uint32_t>("bounds")[0];
        g_search_bound = arr<uint32_t>("bounds")[1];
        swa::DeviceScope scope = swa::DeviceScope::gpu_device(0);
        levenshtein<swa::LevenshteinDistances>("LevenshteinDistances", scope, "b", false);
        levenshtein<swa::LevenshteinDistancesUtf8>("LevenshteinDistancesUtf8", scope, "u", true);
        alignment<swa::NeedlemanWunschScores>("NeedlemanWunschScores", "nw", scope);
        alignment<swa::SmithWatermanScores>("SmithWatermanScores", "sw", scope);
    } catch (const swa::Error &e) {
        std::printf("setup: swa::Error status %d, %s\n", (int)e.status, e.what());
        ++g_failures;
    }
    std::fprintf(stderr, "check_hpp: %d difference%s\n", g_failures, g_failures == 1 ? "" : "s");
    return g_failures ? 1 : 0;
}
