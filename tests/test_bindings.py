"""The C and C++ bindings against the references: include/stringwars_amd.h called from C (tests/bindings/check_c.c), the wrappers of
include/stringwars_amd.hpp called from C++ (tests/bindings/check_hpp.cpp), and the ctypes table of stringwars_amd/_native.py held to
the headers type by type.

This file builds the inputs, computes every expected array with the references the suite already has (the CPU oracle, and the numpy /
pure-Python references of test_align, test_infix, test_osa, test_lcs, test_jaro, test_topk and test_within -- never stringwars_amd
itself), and writes them into one case file that both programs read. The programs compare every output element exactly and print one
line per call and variant: `<name>: ok`, or the first difference.

Case file (little-endian, no padding): the 8 bytes "SWCASE1\\0", a u32 array count, then per array a u32 name length, the name, a u32
dtype code (0 u8, 1 u32, 2 u64, 3 i32, 4 i64, 5 i8), a u64 element count and the elements."""
import ctypes as C
import os
import re
import struct
import subprocess
import time

import numpy as np
import pytest

from test_abi import _HANDLES, _c_parameter_types, declared_symbols
from test_align import reference_script
from test_infix import reference_infix
from test_jaro import reference as reference_jaro
from test_lcs import reference_indel, reference_lcs
from test_osa import reference_osa
from test_topk import expected_topk
from test_within import expected_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PACKAGE = os.path.join(ROOT, "stringwars_amd")
SOURCES = os.path.join(ROOT, "tests", "bindings")
CHECK_HPP, CHECK_C = os.path.join(PACKAGE, "check_hpp"), os.path.join(PACKAGE, "check_c")
HEADERS = ("stringwars_amd.h", "stringwars_amd_harness.h")
NONE = 0xFFFFFFFF

# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
ALPHABETS = {"b": "acgt", "u": "aж中\U0001F600"}   # bytes: acgt; code points: Latin, Cyrillic, CJK, emoji = 1, 2, 3, 4 bytes
PAIRS, LONGEST, BIG, BIG_AT = 300, 100, 2048, 100          # pair BIG_AT has BIG symbols on both sides, pair BIG_AT + 1 has 33 on the shorter
PAIR_BOUND, SEARCH_BOUND = 10, 8
PAIR_VIEW, QUERY_VIEW, CANDIDATE_VIEW = (7, PAIRS - 5), (3, 21), (2, 37)   # subview(lo, hi) of the prepared tapes
QUERIES, CANDIDATES = 24, 40
KS = (1, 5, 64)
DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint32): 1, np.dtype(np.uint64): 2, np.dtype(np.int32): 3, np.dtype(np.int64): 4, np.dtype(np.int8): 5}


class Tape:
    """What the oracle takes: .data (uint8) and .offsets (uint64) of the UTF-8 encodings of `strings`."""

    def __init__(self, strings):
        encoded = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strings]
        self.data = np.frombuffer(b"".join(encoded) + b"\0", dtype=np.uint8)[:-1].copy()
        self.offsets = np.zeros(len(encoded) + 1, dtype=np.uint64)
        np.cumsum([len(e) for e in encoded], out=self.offsets[1:])


def draw(rng, alphabet, n):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def mutated(rng, s, edits, alphabet):
    s = list(s)
    for _ in range(edits):
        op, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(s) + 1))
        if op == 0 and pos < len(s):
            s[pos] = alphabet[int(rng.integers(0, len(alphabet)))]
        elif op == 1:
            s.insert(pos, alphabet[int(rng.integers(0, len(alphabet)))])
        elif pos < len(s):
            del s[pos]
    return "".join(s)


def token_pairs(rng, alphabet):
    """test_tiled_interior.token_pairs over `alphabet`: lengths 0 .. LONGEST with empty and equal strings, mutated copies and unrelated
    strings; then the two long pairs."""
    a_side, b_side = [], []
    for i in range(PAIRS):
        a = draw(rng, alphabet, int(rng.integers(0, LONGEST + 1)))
        kind = i % 8
        if kind == 0:
            b = a
        elif kind == 1:
            b = "" if i % 16 == 1 else a[: len(a) // 2]
        elif kind < 4:
            b = mutated(rng, a, int(rng.integers(1, 7)), alphabet)
        else:
            b = draw(rng, alphabet, int(rng.integers(0, LONGEST + 1)))
        if kind == 7 and i % 16 == 7:
            a = ""
        a_side.append(a)
        b_side.append(b)
    big = draw(rng, alphabet, BIG)
    other = list(big)
    for pos in rng.integers(0, BIG, 40):                      # substitutions and one swap of neighbours: both sides keep BIG symbols
        other[pos] = alphabet[int(rng.integers(0, len(alphabet)))]
    other[1000], other[1001] = other[1001], other[1000]
    a_side[BIG_AT], b_side[BIG_AT] = big, "".join(other)
    a_side[BIG_AT + 1] = draw(rng, alphabet, 33)
    b_side[BIG_AT + 1] = mutated(rng, a_side[BIG_AT + 1], 5, alphabet) + draw(rng, alphabet, 9)
    return a_side, b_side


def search_strings(rng, alphabet):
    """Candidates of at most SEARCH_BOUND symbols, so the empty query has a full row; a query of one far symbol repeated has an empty
    one; of the rest a quarter are mutated candidates (nearly full rows), the others unrelated strings of 10 to 24 symbols (few hits)."""
    candidates = [draw(rng, alphabet, int(rng.integers(0, SEARCH_BOUND + 1))) for _ in range(CANDIDATES)]
    queries = []
    for i in range(QUERIES):
        if i % 4 == 0:
            queries.append(mutated(rng, candidates[int(rng.integers(0, CANDIDATES))], int(rng.integers(0, 4)), alphabet))
        else:
            queries.append(draw(rng, alphabet, int(rng.integers(10, 25))))
    queries[5], queries[11] = "", alphabet[3] * 30
    return queries, candidates


def put_tape(case, name, strings):
    tape = Tape(strings)
    case[name + ".data"], case[name + ".off"] = tape.data, tape.offsets
    return tape


def dense(queries, candidates, utf8):
    """Every dense matrix of queries x candidates, from the references, as (nq, nc) int64 arrays."""
    nq, nc = len(queries), len(candidates)
    rows, columns = [q for q in queries for _ in candidates], [c for _ in queries for c in candidates]
    import oracle
    lcs = reference_lcs(rows, columns, utf8)
    jaro = reference_jaro(rows, columns, utf8)
    out = {"lev": oracle.levenshtein_pairs(Tape(rows), Tape(columns), utf8=utf8), "osa": reference_osa(rows, columns, utf8), "lcs": lcs,
           "indel": reference_indel(rows, columns, utf8, lcs=lcs), "jaro_m": jaro[:, 0], "jaro_t": jaro[:, 1], "jaro_p": jaro[:, 2]}
    return {key: np.asarray(value, dtype=np.int64).reshape(nq, nc) for key, value in out.items()}


def put_search(case, name, d):
    for k in KS:
        for tag, bound in (("u", None), ("b", SEARCH_BOUND)):
            indices, distances = expected_topk(d, k, bound)
            case[f"{name}.topk.k{k}.{tag}.i"], case[f"{name}.topk.k{k}.{tag}.d"] = indices.ravel(), distances.ravel()
    offsets, indices, distances = expected_csr(d, SEARCH_BOUND)
    case[name + ".within.off"], case[name + ".within.i"], case[name + ".within.d"] = offsets, indices, distances


def levenshtein_case(case, prefix, seed):
    import oracle
    utf8, alphabet = prefix == "u", ALPHABETS[prefix]
    rng = np.random.default_rng(seed)
    a, b = token_pairs(rng, alphabet)
    ta, tb = put_tape(case, prefix + ".pa", a), put_tape(case, prefix + ".pb", b)
    u32 = lambda x: np.asarray(x, dtype=np.int64).astype(np.uint32)
    clamp = lambda x: np.minimum(np.asarray(x, dtype=np.int64), PAIR_BOUND + 1)
    lev = np.asarray(oracle.levenshtein_pairs(ta, tb, utf8=utf8), dtype=np.int64)
    case[prefix + ".lev"], case[prefix + ".lev_b"] = u32(lev), u32(clamp(lev))
    osa = reference_osa(a, b, utf8)
    case[prefix + ".osa"], case[prefix + ".osa_b"] = u32(osa), u32(clamp(osa))
    lcs = reference_lcs(a, b, utf8)
    indel = reference_indel(a, b, utf8, lcs=lcs)
    case[prefix + ".lcs"], case[prefix + ".indel"], case[prefix + ".indel_b"] = u32(lcs), u32(indel), u32(clamp(indel))
    jaro = reference_jaro(a, b, utf8)
    for column, key in enumerate(("jaro_m", "jaro_t", "jaro_p")):
        case[f"{prefix}.{key}"] = u32(jaro[:, column])
    # infix: pattern a_i in text b_i; over the bound: (bound + 1, NONE, NONE), as the header states
    found = np.array([reference_infix(p, t, utf8) for p, t in zip(a, b)], dtype=np.int64).reshape(PAIRS, 3)
    over = found[:, 0] > PAIR_BOUND
    for column, key in enumerate(("infix_d", "infix_s", "infix_e")):
        case[f"{prefix}.{key}"] = u32(found[:, column])
        case[f"{prefix}.{key}_b"] = u32(np.where(over, PAIR_BOUND + 1 if column == 0 else NONE, found[:, column]))
    # alignments: the canonical script; over the bound: distance bound + 1 and an empty range
    scripts = [reference_script(x, y, utf8) for x, y in zip(a, b)]
    assert [d for d, _ in scripts] == lev.tolist()
    for tag, kept in (("", [ops for _, ops in scripts]), ("_b", [ops if d <= PAIR_BOUND else b"" for d, ops in scripts])):
        offsets = np.zeros(PAIRS + 1, dtype=np.uint64)
        np.cumsum([len(ops) for ops in kept], out=offsets[1:])
        case[f"{prefix}.align_off{tag}"] = offsets
        case[f"{prefix}.align_ops{tag}"] = np.frombuffer(b"".join(kept) + b"\0", dtype=np.uint8)[:-1].copy()
    case[prefix + ".ops_capacity"] = np.array([len(ta.data) + len(tb.data)], dtype=np.uint64)
    # the searches and the dense products: queries x candidates (x), queries x queries (s), and for the subviews vx and vs
    queries, candidates = search_strings(rng, alphabet)
    put_tape(case, prefix + ".q", queries)
    put_tape(case, prefix + ".c", candidates)
    (ql, qh), (cl, ch) = QUERY_VIEW, CANDIDATE_VIEW
    for name, d in (("x", dense(queries, candidates, utf8)), ("s", dense(queries, queries, utf8))):
        for key, matrix in d.items():
            case[f"{prefix}.{name}.{key}"] = matrix.astype(np.uint64).ravel()
        put_search(case, f"{prefix}.{name}", d["lev"])
        put_search(case, f"{prefix}.v{name}", d["lev"][ql:qh, cl:ch] if name == "x" else d["lev"][ql:qh, ql:qh])
    # the inputs are what they are for (so no check passes vacuously)
    shorter = [min(len(x), len(y)) for x, y in zip(a, b)]
    assert shorter[BIG_AT] == BIG and shorter[BIG_AT + 1] == 33 and "" in a and "" in b and any(x == y and x for x, y in zip(a, b))
    assert (lev > PAIR_BOUND).sum() > 30 and (lev <= PAIR_BOUND).sum() > 30 and over.any() and not over.all()
    assert (np.asarray(osa) != lev).any() and PAIR_VIEW[0] < BIG_AT < PAIR_VIEW[1]
    hits = case[f"{prefix}.x.lev"].reshape(QUERIES, CANDIDATES).astype(np.int64) <= SEARCH_BOUND
    assert 0.15 <= hits.mean() <= 0.40, hits.mean()                  # about a quarter of the entries qualify
    assert (hits.sum(axis=1) == 0).any() and hits.all(axis=1).any()  # one row empty, one full
    assert max(KS) > CANDIDATES > QUERIES and all(2 <= int(case[f"{prefix}.{p}.within.off"][-1]) for p in ("x", "s", "vx", "vs"))


def alignment_case(case, seed=7):
    """NW / SW: 64 pairs of up to 200 amino-acid letters and a 12 x 9 product, gaps (-4, -4) and (-11, -1), a 32-class table (expanded
    here to the 256 x 256 matrix it stands for) and a full 256 x 256 matrix."""
    import oracle
    rng = np.random.default_rng(seed)
    letters = "ACDEFGHIKLMNPQRSTVWY"
    a = [draw(rng, letters, int(rng.integers(0 if i % 16 == 0 else 1, 201))) for i in range(64)]
    b = [mutated(rng, x, int(rng.integers(0, 30)), letters) if i % 2 else draw(rng, letters, int(rng.integers(1, 201))) for i, x in enumerate(a)]
    queries, candidates = a[20:32], b[3:12]
    tapes = {name: put_tape(case, "nw." + name, strings) for name, strings in (("pa", a), ("pb", b), ("q", queries), ("c", candidates))}
    classes = ((np.arange(256) * 7 + 3) % 32).astype(np.uint8)
    costs = rng.integers(-4, 4, (32, 32)).astype(np.int8)
    costs = np.triu(costs) + np.triu(costs, 1).T
    costs[np.arange(32), np.arange(32)] = rng.integers(4, 12, 32)
    full = rng.integers(-4, 4, (256, 256)).astype(np.int8)
    full = np.triu(full) + np.triu(full, 1).T
    full[np.arange(256), np.arange(256)] = rng.integers(4, 12, 256)
    case["nw.classes"], case["nw.costs"], case["nw.matrix"] = classes, costs.ravel(), full.ravel()
    assert len({int(classes[ord(x)]) for x in letters}) == len(letters)
    expand = lambda left, right: (Tape([x for x in left for _ in right]), Tape([y for _ in left for y in right]))
    products = {"pairs": (tapes["pa"], tapes["pb"]), "cross": expand(queries, candidates), "self": expand(queries, queries)}
    for engine, matrix in (("classes", costs[classes][:, classes]), ("matrix", full)):
        for gaps, (gap_open, gap_extend) in (("linear", (-4, -4)), ("affine", (-11, -1))):
            for shape, (left, right) in products.items():
                dtype = np.int32 if shape == "pairs" else np.int64
                count = len(left.offsets) - 1
                case[f"nw.{engine}.{gaps}.{shape}"] = np.asarray(oracle.nw_pairs(left, right, matrix, gap_open, gap_extend)).astype(dtype)
                local = [oracle.nw_score(bytes(left.data[int(left.offsets[i]):int(left.offsets[i + 1])]), bytes(right.data[int(right.offsets[i]):int(right.offsets[i + 1])]),
                                         matrix, gap_open, gap_extend, local=True) for i in range(count)]
                case[f"sw.{engine}.{gaps}.{shape}"] = np.array(local, dtype=dtype)


def refusal_case(case):
    """A pair whose both sides hold one symbol more than each per-call limit allows (all four limits are 2048), and a tape with a
    stray continuation byte."""
    put_tape(case, "long.a", ["ac" * 1024 + "g", "acgt"])
    put_tape(case, "long.b", ["ca" * 1024 + "t", "acgt"])
    put_tape(case, "bad.a", [b"abc", b"a\x80c", b"xyz"])
    put_tape(case, "bad.b", [b"abd", b"abc", b"xyz"])


_CASE = {}


def the_case():
    """Computed once per session and shared, unchanged, by the tests that need it."""
    if not _CASE:
        levenshtein_case(_CASE, "b", seed=11)
        levenshtein_case(_CASE, "u", seed=12)
        alignment_case(_CASE)
        refusal_case(_CASE)
        _CASE["bounds"] = np.array([PAIR_BOUND, SEARCH_BOUND], dtype=np.uint32)
        _CASE["views"] = np.array(PAIR_VIEW + QUERY_VIEW + CANDIDATE_VIEW, dtype=np.uint64)
    return _CASE


def write_case(path, case):
    with open(path, "wb") as out:
        out.write(b"SWCASE1\0" + struct.pack("<I", len(case)))
        for name, array in case.items():
            array = np.ascontiguousarray(array)
            out.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<IQ", DTYPES[array.dtype], array.size) + array.tobytes())


def tiny_case(path):
    """What the no-device pass reads: the two refusal tapes are all it needs."""
    case = {}
    refusal_case(case)
    write_case(path, case)


# ---- what the programs must report --------------------------------------------------------------------------------------------------
FORMS = ("raw", "prepared", "subview")
BOUNDS = ("unbounded", "bound")
SHAPES = [f"{c}|{s}" for c in ("self", "candidates") for s in ("packed", "stride")]
VARIANTS = {
    "pairs_into": BOUNDS, "osa": BOUNDS, "infix": BOUNDS, "align": BOUNDS,
    "lcs": [f"{o}|{b}" for o in ("both", "indel", "lcs") for b in BOUNDS],
    "jaro": ["all", "matches", "transpositions", "prefix"],
    "compute_into": SHAPES, "osa_cross": SHAPES,
    "lcs_cross": [f"{o}|{s}" for o in ("both", "indel", "lcs") for s in SHAPES],
    "jaro_cross": [f"{o}|{s}" for o in ("all", "matches", "transpositions", "prefix") for s in SHAPES],
    "topk": [f"{c}|k{k}|{b}" for c in ("self", "candidates") for k in KS for b in BOUNDS],
    "within": [f"{c}|{m}" for c in ("self", "candidates") for m in ("count", "exact", "short")],
}
ALIGNMENT_VARIANTS = {
    "pairs_into": [f"{e}|{g}" for e in ("classes", "matrix") for g in ("linear", "affine")],
    "compute_into": [f"{e}|{g}|{s}" for e in ("classes", "matrix") for g in ("linear", "affine") for s in SHAPES],
}
# wrapper overloads this file does not run, each with its reason
NOT_RUN = {"ShardedCross": "needs a multi-device scope: tests/test_sharding.py", "ShardedPairs": "needs a multi-device scope: tests/test_sharding.py"}
FORM_OF = {"BytesTapeView": ("raw",), "PreparedTape": ("prepared", "subview")}


def wrapper_methods(text=None):
    """{class: {(method, type of its first tape)}} of the engine classes of stringwars_amd.hpp, by regex, in the style of
    test_abi.declared_symbols: every `void name(const DeviceScope &scope, const <Tape> &...` between `class X` and the next class."""
    text = text if text is not None else open(os.path.join(INCLUDE, "stringwars_amd.hpp")).read()
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for match in re.finditer(r"\nclass (\w+)[^{;]*\{(.*?)\n\};", text, flags=re.S):
        methods = set(re.findall(r"\bvoid (\w+)\(const DeviceScope &\w+, const (\w+) &", match.group(2)))
        if methods:
            found[match.group(1)] = methods
    return found


def expected_lines(text=None):
    """Every `name` the C++ program must report `ok` for; a wrapper with no entry in VARIANTS gets a name nothing reports."""
    methods = wrapper_methods(text)
    assert set(methods) == {"LevenshteinDistances", "NeedlemanWunschScores", "SmithWatermanScores"}, sorted(methods)
    lines = []
    for cls, found in sorted(methods.items()):
        table = VARIANTS if cls == "LevenshteinDistances" else ALIGNMENT_VARIANTS
        for method, tape in sorted(found):
            if tape in NOT_RUN:
                continue
            for form in FORM_OF.get(tape, ("unknown-tape-type",)):
                for variant in table.get(method, ("no-check-for-this-wrapper",)):
                    for name in ((cls, cls + "Utf8") if cls == "LevenshteinDistances" else (cls,)):
                        lines.append(f"{name}.{method}[{form}|{variant}]")
    return lines


C_CHECKS = [
    "u32tape.levenshtein_pairs", "u32tape.levenshtein_utf8_pairs", "u32tape.nw_pairs", "u32tape.sw_pairs", "u32tape.prepare_u32",
    "prepared.nw_pairs", "prepared.nw_cross", "prepared.sw_pairs", "prepared.sw_cross",
    "stride8.levenshtein_pairs", "stride8.osa_pairs", "stride8.lcs_pairs", "stride8.nw_pairs", "stride12.jaro_pairs",
    "device_alloc.levenshtein_pairs", "unified_alloc.levenshtein_pairs", "device_alloc.jaro_cross",
    "async.synchronize", "pipelined.join", "describe.short", "forget.again", "version", "capabilities",
    "refuse.null_engine.levenshtein_pairs", "refuse.null_engine.topk", "refuse.null_engine.infix", "refuse.null_engine.osa_pairs",
    "refuse.counts.levenshtein_pairs", "refuse.counts.align", "refuse.counts.infix", "refuse.counts.osa_pairs", "refuse.counts.lcs_pairs",
    "refuse.counts.jaro_pairs", "refuse.counts.nw_pairs",
    "refuse.utf8.levenshtein_pairs", "refuse.utf8.prepare", "refuse.utf8.align", "refuse.utf8.infix", "refuse.utf8.osa_pairs",
    "refuse.utf8.lcs_pairs", "refuse.utf8.jaro_pairs", "refuse.utf8.topk", "refuse.utf8.within",
    "refuse.length.infix", "refuse.length.osa_pairs", "refuse.length.lcs_pairs", "refuse.length.jaro_pairs",
]


def reported(stdout):
    return dict(line.rsplit(": ", 1) if ": " in line else (line, "") for line in stdout.splitlines())


def run_program(binary, case_path):
    done = subprocess.run([binary, str(case_path)], capture_output=True, text=True, timeout=120)
    return done, reported(done.stdout)


# ---- CPU: the ctypes table against the headers, with types -----------------------------------------------------------------------------
_STRUCTS = {"swh_tape_u32_t": "TapeU32", "swh_tape_u64_t": "TapeU64", "swh_prepared_view_t": "PreparedView", "swh_prepared_info_t": "PreparedInfo",
            "swh_timing_t": "Timing", "swh_timing_totals_t": "TimingTotals", "swh_shard_timing_t": "ShardTiming", "swh_synth_t": "Synth"}
# header structs without a ctypes class, ctypes classes without a header struct: none today
STRUCT_ALLOW_LIST = {}


def _c_to_ctypes():
    from stringwars_amd import _native as N
    table = {
        "int": (C.c_int,), "swh_algorithm_t": (C.c_int,), "swh_status_t": (C.c_int,), "size_t": (C.c_size_t,), "uint32_t": (C.c_uint32,),
        "uint64_t": (C.c_uint64,), "int8_t": (C.c_int8,), "double": (C.c_double,), "void": (None,),
        "const char *": (C.c_char_p,), "char *": (C.c_char_p, C.c_void_p), "const char **": (C.POINTER(C.c_char_p),),
        "void *": (C.c_void_p,), "const void *": (C.c_void_p,), "void **": (C.POINTER(C.c_void_p),),
    }
    # a typed data pointer: the pointer to its ctypes type, or void *
    for c_type, element in (("int", C.c_int), ("size_t", C.c_size_t), ("ptrdiff_t", C.c_ssize_t), ("uint32_t", C.c_uint32), ("int32_t", C.c_int32),
                            ("int8_t", C.c_int8), ("uint8_t", C.c_uint8), ("uint64_t", C.c_uint64)):
        table[c_type + " *"] = table["const " + c_type + " *"] = (C.POINTER(element), C.c_void_p)
    for c_type, name in _STRUCTS.items():
        table[c_type + " *"] = table["const " + c_type + " *"] = (C.POINTER(getattr(N, name)),)
    for handle in _HANDLES:
        table[handle] = (C.c_void_p,)
        table[handle + " *"] = (C.POINTER(C.c_void_p),)
    return table


def _same_ctype(found, wanted):
    """ctypes keeps one class per C type (c_size_t IS c_uint64 on LP64, POINTER(x) is cached), so identity is the C type's identity."""
    return found is wanted


def header_text(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def ctypes_abi_mismatches(text, signatures, names):
    """Every (symbol, position or 'count' / 'return' / 'declaration', C type, ctypes type found) where the ctypes table and the header
    differ. `void *` in the table stands for any typed DATA pointer of the header; a scalar never stands for another."""
    table, wrong = _c_to_ctypes(), []
    for name in names:
        declaration = re.search(r"([A-Za-z_][A-Za-z_0-9 ]*?[ \*]+)%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        if not declaration or name not in signatures:
            wrong.append((name, "declaration", None, None))
            continue
        c_types = _c_parameter_types(declaration.group(2))
        restype, argtypes = signatures[name]
        if len(c_types) != len(argtypes):
            wrong.append((name, "count", len(c_types), len(argtypes)))
            continue
        for position, (c_type, found) in enumerate(zip(c_types, argtypes)):
            if not any(_same_ctype(found, wanted) for wanted in table.get(c_type, ())):
                wrong.append((name, position, c_type, found))
        c_return = " ".join(declaration.group(1).replace("*", " * ").split()).replace(" *", " *")
        if not any(_same_ctype(restype, wanted) for wanted in table.get(c_return, ())):
            wrong.append((name, "return", c_return, restype))
    return wrong


def test_ctypes_table_matches_the_headers_with_types(sw):
    from stringwars_amd import _native as N
    for header in HEADERS:
        text, names = header_text(header), declared_symbols(header)
        assert not ctypes_abi_mismatches(text, N.SIGNATURES, names), ctypes_abi_mismatches(text, N.SIGNATURES, names)
    text, names = header_text("stringwars_amd.h"), declared_symbols("stringwars_amd.h")
    # the check has teeth: size_t <-> uint32_t both ways, a dropped parameter and a changed return type are each caught
    def seeded(name, change):
        restype, argtypes = N.SIGNATURES[name]
        return dict(N.SIGNATURES, **{name: change(restype, list(argtypes))})
    narrowed = seeded("swh_levenshtein_topk_u64tape", lambda r, a: (r, a[:4] + [C.c_uint32] + a[5:]))      # k: size_t -> uint32_t
    assert [w[:2] for w in ctypes_abi_mismatches(text, narrowed, names)] == [("swh_levenshtein_topk_u64tape", 4)]
    widened = seeded("swh_levenshtein_pairs_u64tape", lambda r, a: (r, a[:4] + [C.c_size_t] + a[5:]))      # bound: uint32_t -> size_t
    assert [w[:2] for w in ctypes_abi_mismatches(text, widened, names)] == [("swh_levenshtein_pairs_u64tape", 4)]
    dropped = seeded("swh_sharded_cuts", lambda r, a: (r, a[:-1]))
    assert [w[:2] for w in ctypes_abi_mismatches(text, dropped, names)] == [("swh_sharded_cuts", "count")]
    returned = seeded("swh_version", lambda r, a: (C.c_int, a))
    assert [w[:2] for w in ctypes_abi_mismatches(text, returned, names)] == [("swh_version", "return")]
    scalar = seeded("swh_scope_set_async", lambda r, a: (r, [a[0], C.c_void_p]))                           # void * never stands for a scalar
    assert [w[:2] for w in ctypes_abi_mismatches(text, scalar, names)] == [("swh_scope_set_async", 1)]


def compile_c(source_text, tmp_path, name, flags=()):
    source = tmp_path / (name + ".c")
    source.write_text(source_text)
    binary = tmp_path / name
    subprocess.run(["gcc", *flags, "-I", INCLUDE, str(source), "-o", str(binary)], check=True, capture_output=True, text=True, timeout=120)
    return binary


def header_structs():
    """{struct: [fields]} of the public structs of both headers (`typedef struct name { ... } name;`)."""
    structs = {}
    for header in HEADERS:
        for body, name in re.findall(r"typedef struct \w+\s*\{(.*?)\}\s*(\w+)\s*;", header_text(header), flags=re.S):
            fields = []
            for statement in body.split(";"):
                if statement.strip():
                    fields += [re.sub(r"\[.*?\]", "", part).split()[-1].lstrip("*") for part in statement.replace("*", " * ").split(",")]
            structs[name] = fields
    return structs


def test_struct_layouts_match_ctypes(sw, tmp_path):
    from stringwars_amd import _native as N
    structs = header_structs()
    assert set(structs) - set(STRUCT_ALLOW_LIST) == set(_STRUCTS), set(structs) ^ set(_STRUCTS)
    classes = {name for name, value in vars(N).items() if isinstance(value, type) and issubclass(value, C.Structure) and value is not C.Structure}
    assert classes - set(STRUCT_ALLOW_LIST) == set(_STRUCTS.values()), classes ^ set(_STRUCTS.values())
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stringwars_amd.h"', '#include "stringwars_amd_harness.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {field} %zu\\n", offsetof({name}, {field}));' for field in fields]
    lines += ["    return 0;", "}"]
    binary = compile_c("\n".join(lines) + "\n", tmp_path, "layout", ("-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror"))
    measured = {}
    for line in subprocess.run([str(binary)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines():
        name, field, value = line.split()
        measured.setdefault(name, {})[field] = int(value)
    for name, fields in structs.items():
        cls = getattr(N, _STRUCTS[name])
        assert [f[0] for f in cls._fields_] == fields, (name, fields)
        assert C.sizeof(cls) == measured[name]["sizeof"], name
        for field in fields:
            assert getattr(cls, field).offset == measured[name][field], (name, field)


@pytest.mark.parametrize("standard", ["c99", "c11"])
def test_headers_compile_as_strict_c(tmp_path, standard):
    source = '#include "stringwars_amd.h"\n#include "stringwars_amd_harness.h"\nint main(void) { return SWH_VERSION_MAJOR; }\n'
    source_file = tmp_path / "strict.c"
    source_file.write_text(source)
    done = subprocess.run(["gcc", f"-std={standard}", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-c", str(source_file), "-o",
                           str(tmp_path / "strict.o")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr


def test_hpp_compiles_as_strict_cpp17(tmp_path):
    source_file = tmp_path / "strict.cpp"
    source_file.write_text('#include "stringwars_amd.hpp"\nint main() { return 0; }\n')
    done = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-c", str(source_file), "-o",
                           str(tmp_path / "strict.o")], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr


def test_the_wrapper_list_is_read_from_the_header():
    """The method list comes from the header: a wrapper added there without a check here gives a line that nothing reports."""
    lines = expected_lines()
    assert len(lines) == len(set(lines)) and "LevenshteinDistancesUtf8.within[subview|candidates|short]" in lines
    assert "SmithWatermanScores.compute_into[raw|matrix|affine|self|stride]" in lines
    hpp = open(os.path.join(INCLUDE, "stringwars_amd.hpp")).read()
    grown = hpp.replace("    void osa(const DeviceScope &scope, const BytesTapeView &a,", "    void hamming(const DeviceScope &scope, const BytesTapeView &a,", 1)
    assert grown != hpp and "LevenshteinDistances.hamming[raw|no-check-for-this-wrapper]" in expected_lines(grown)
    assert all(not line.endswith("no-check-for-this-wrapper]") and "unknown-tape-type" not in line for line in lines)


def no_device():
    import torch
    return not torch.cuda.is_available()


NO_DEVICE_HPP = ["nodevice.DeviceScope.gpu_device", "nodevice.DeviceScope.gpu_devices", "nodevice.DeviceScope.cpu_cores", "nodevice.PreparedTape",
                 "nodevice.LevenshteinDistances", "nodevice.LevenshteinDistancesUtf8", "nodevice.NeedlemanWunschScores.classes",
                 "nodevice.NeedlemanWunschScores.matrix", "nodevice.SmithWatermanScores.classes", "nodevice.SmithWatermanScores.matrix",
                 "nodevice.ShardedPairs", "nodevice.ShardedCross"]


def check_no_device_run(binary, tmp_path, names):
    case_path = tmp_path / "tiny.case"
    tiny_case(case_path)
    done, lines = run_program(binary, case_path)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-2000:]
    bad = {name: text for name, text in lines.items() if text != "ok"}
    assert not bad, bad
    missing = [name for name in names if name not in lines]
    assert not missing, missing
    return lines


@pytest.mark.skipif(not (os.path.exists(CHECK_HPP) and os.path.exists(CHECK_C)), reason="check_hpp / check_c not built")
def test_programs_refuse_every_call_without_a_device(tmp_path):
    """Every entry point of stringwars_amd.h, called once from C with null handles (no handle can exist without a device), returns the
    status the header documents, sets a message where it has an `error` parameter and leaves its outputs at their sentinel; every
    constructor of the C++ header throws that status. (A C++ engine cannot be constructed without a device, so its methods are not
    reachable here: they run on the GPU.)"""
    if not no_device():
        pytest.skip("a GPU is present; covered by the gpu tests")
    check_no_device_run(CHECK_HPP, tmp_path, NO_DEVICE_HPP)
    lines = check_no_device_run(CHECK_C, tmp_path, ["nodevice." + name for name in declared_symbols("stringwars_amd.h")])
    assert len(lines) >= len(declared_symbols("stringwars_amd.h"))


def test_programs_under_host_sanitizers_without_a_device(tmp_path):
    """Both programs built again with -fsanitize=address,undefined (the programs and the header's inline code; the library as built)
    and run through the no-device pass. Stand-alone executables: nothing is preloaded."""
    if not no_device():
        pytest.skip("host-side sanitizers run on the CPU machine only")
    link = ["-I", INCLUDE, "-L", PACKAGE, "-lstringwars_amd", f"-Wl,-rpath,{PACKAGE}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
    programs = ((["g++", "-std=c++17"], "check_hpp.cpp", NO_DEVICE_HPP), (["gcc", "-std=c99"], "check_c.c", ["nodevice.swh_scope_init_gpu"]))
    for compiler, source, names in programs:
        binary = tmp_path / (source.split(".")[0] + "_sanitized")
        subprocess.run([*compiler, *sanitize, "-Wall", os.path.join(SOURCES, source), "-o", str(binary), *link], check=True, capture_output=True,
                       text=True, timeout=300)
        check_no_device_run(str(binary), tmp_path, names)


# ---- GPU: both programs against the case file -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(not (os.path.exists(CHECK_HPP) and os.path.exists(CHECK_C)), reason="check_hpp / check_c not built (make -C stringwars_amd/csrc)")
def test_c_and_cpp_bindings_against_the_references(tmp_path):
    began = time.perf_counter()
    case_path = tmp_path / "bindings.case"
    write_case(case_path, the_case())
    wrote = time.perf_counter()
    for binary, names in ((CHECK_HPP, expected_lines()), (CHECK_C, C_CHECKS)):
        done, lines = run_program(binary, case_path)
        bad = {name: text for name, text in lines.items() if text != "ok"}
        assert not bad, (os.path.basename(binary), list(bad.items())[:12], done.stderr[-2000:])
        assert done.returncode == 0, (os.path.basename(binary), done.returncode, done.stdout[-2000:], done.stderr[-2000:])
        missing = [name for name in names if name not in lines]
        assert not missing, (os.path.basename(binary), len(missing), missing[:12])
    print(f"bindings: references and case file {wrote - began:.2f} s, both programs {time.perf_counter() - wrote:.2f} s, "
          f"{len(expected_lines())} C++ checks, {len(C_CHECKS)} C checks")
