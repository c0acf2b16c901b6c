"""Cases, inputs, fp64 references, the route mirror and the comparison of test_gpu_match_routes.py (host only;
test_match_route_checks_cpu.py shows that the inputs leave no decision near flipping, that the comparison accepts the fp32
oracle and that it rejects the faults a confidence pass is likely to have, on this very data).

The dense matcher (csrc/match.hip, csrc/sinkhorn.hip) picks its confidence pass from S alone (launch_conf_pass):
  odd S         conf_pass_kernel<PUBLISH>: single columns, chunks of 1024, a RowBest per row merged across chunks
  even S        conf_pass_fast_kernel<PUBLISH, NK>, NK = 4 / 8 / 12 / 16 for S <= 512 / 1024 / 1536 / 2048: one chunk
  even S > 2048 the NK = 16 kernel over chunks of 2048; lane 0 merges a row's chunk results through global memory
  Sinkhorn      skh_conf_kernel: chunks of 1024, either parity
Rows come in blocks of 32 (8 per wave; the fast kernel fetches them in pairs, one row ahead); select_kernel tests a row's
argmax column against the column maxima and re-scans the row in steps of 64 columns when its maximum is tied; scatter_kernel
compacts in rounds of 256 rows.  `want_conf=False` runs the non-PUBLISH twins, whose re-scan recomputes conf from sim.

Inputs: f0, f1 ~ N(0, 1) (C = 64), K = min(L, S) injective (row, column) pairs planted with noise 0.1: with temperature 0.1 a
planted pair scores ~10 in sim against N(0, 1.25^2), so matched confidences spread over ~0.2 .. 1.0 (they depend on |f0_i|^2
and on S) instead of saturating at 1.000, and a wrong column statistic or a dropped chunk moves values the comparison sees.
Reference: oracle/coarse_match_ref.py (dual softmax) / pope_amd/sinkhorn_cpu.py (Sinkhorn) on the inputs cast to double, pushed
through coarse_match.  Bounds: rtol 1e-4, atol 1e-7 on mconf and on the whole conf_matrix, what test_gpu_match.py and
test_gpu_sinkhorn.py hold the matcher to.

Tie cases overwrite an unplanted column j' of a LATER chunk with a column j of chunk 0 that is planted for an interior row i, so
that row i has two bit-equal maxima in different chunks.  Variant a: j interior, the first maximum wins (j_id = j).  Variant b:
j inside the top border of grid 1, so only a re-scan that walks on into the later chunk finds j_id = j'.  Where the later chunk
holds border columns only (S = 2050: columns 2048, 2049 lie in the last grid row; S = 1025: column 1024 is the last cell), j'
is a border column: variant a still expects j, variant b expects no match for row i after a re-scan over every chunk.  The
reference enforces the mathematical tie (conf64[:, :, j'] = conf64[:, :, j]); the clear-decision sets treat the twin columns as
one column (the choice between them is an exact rule, not a margin).

Sinkhorn cases follow pope_amd.synth.sinkhorn_case (C = 256, N(0, 1), 60 % planted with noise 0.3, scaled by sqrt(12),
bin_score 1.0, 3 iterations, prefilter on).  Its tie case alone runs with the prefilter off: two identical columns share row i's
unit of mass (0.47 each), each column's dustbin takes the other 0.53, and the prefilter would zero both columns."""
import math

import numpy as np
import torch

from oracle import coarse_match_ref as cm
from pope_amd import sinkhorn_cpu

RTOL, ATOL = 1e-4, 1e-7
CLEAR = 1e-3          # tests/test_gpu_loftr.py: a decision is clear when every margin exceeds this
THR, TEMPERATURE = 0.2, 0.1
N_PAIRS = 2
C_DS, C_SKH = 64, 256
SKH_BIN_SCORE, SKH_ITERS = 1.0, 3
LIST_KEYS = ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c")

CP_ROWS = 32          # match.hip / sinkhorn.hip: rows per workgroup
FAST_CHUNK, ODD_CHUNK, SKH_CHUNK = 2048, 1024, 1024


# ---- route mirror -----------------------------------------------------------------------------------------------------------
def chunk_of(kind, S):
    """Columns per chunk of the confidence pass that serves S."""
    if kind == "skh":
        return SKH_CHUNK
    return ODD_CHUNK if S & 1 else FAST_CHUNK


def route(kind, L, S):
    """launch_conf_pass (match.hip) / pope_launch_sinkhorn_passes (sinkhorn.hip) restated: (kernel, NK or None, chunks, row blocks)."""
    blocks = -(-L // CP_ROWS)
    if kind == "skh":
        return ("skh_conf_kernel", None, -(-S // SKH_CHUNK), blocks)
    if S & 1:
        return ("conf_pass_kernel", None, -(-S // ODD_CHUNK), blocks)
    nk = -(-S // 128)
    nk = 4 if nk <= 4 else 8 if nk <= 8 else 12 if nk <= 12 else 16
    return ("conf_pass_fast_kernel", nk, -(-S // (128 * nk)), blocks)


def route_name(c):
    k, nk, chunks, blocks = route(c["kind"], c["L"], c["S"])
    return f"{k}{f'<NK={nk}>' if nk else ''} x {chunks} chunk{'s' * (chunks > 1)}, {blocks} row block{'s' * (blocks > 1)}"


# ---- the case table ---------------------------------------------------------------------------------------------------------
def _case(kind, hw0, hw1, pins, border=2, tie=None, seed=None, prefilter=True):
    """seed None: 1000 + the case's place in ALL_CASES.  prefilter: skh_prefilter (Sinkhorn cases)."""
    L, S = hw0[0] * hw0[1], hw1[0] * hw1[1]
    name = f"{kind}-{hw0[0]}x{hw0[1]}_vs_{hw1[0]}x{hw1[1]}-L{L}-S{S}-b{border}" + (f"-tie_{tie}" if tie else "")
    return dict(id=name, kind=kind, hw0=hw0, hw1=hw1, L=L, S=S, border=border, tie=tie, seed=seed, pins=pins, prefilter=prefilter)


G0 = (7, 9)           # L = 63: two row blocks, the second ragged (31 rows: an odd tail for the pairwise row fetch)
COLUMN_CASES = [
    _case("ds", G0, (16, 32), "NK=4, full: S = 512"),
    _case("ds", G0, (12, 43), "first NK=8: S = 516"),
    _case("ds", G0, (32, 32), "NK=8, full: S = 1024"),
    _case("ds", G0, (27, 38), "first NK=12: S = 1026"),
    _case("ds", G0, (32, 48), "NK=12, full: S = 1536"),
    _case("ds", G0, (35, 44), "first NK=16: S = 1540"),
    _case("ds", G0, (32, 64), "NK=16, one exact chunk: S = 2048"),
    _case("ds", G0, (41, 50), "NK=16, second chunk of 2 columns: S = 2050"),
    _case("ds", G0, (50, 82), "NK=16, three chunks, the last of 4 columns: S = 4100"),
    _case("ds", G0, (31, 33), "odd, one ragged chunk: S = 1023"),
    _case("ds", G0, (25, 41), "odd, second chunk of 1 column: S = 1025"),
    _case("ds", G0, (17, 121), "odd, three chunks: S = 2057"),
]
ROW_CASES = [_case("ds", g0, g1, f"{pins}; {'fast' if g1 == (10, 13) else 'odd'} kernel", border=0)
             for g1 in ((10, 13), (9, 11))
             for g0, pins in (((1, 1), "single row: L = 1"),
                              ((1, 7), "odd, less than one wave's 8 rows: L = 7"),
                              ((3, 11), "one row in the second block: L = 33"),
                              ((5, 13), "odd tail in the third block: L = 65"))]
MANY_ROW_CASES = [
    _case("ds", (41, 50), (7, 9), "65 row blocks, nine compaction rounds; odd S = 63"),
    _case("ds", (41, 50), (10, 13), "65 row blocks, nine compaction rounds; NK=4"),
    # (seed searched: ~2450 matches leave about four confidences within CLEAR of thr at a typical seed)
    _case("ds", (41, 50), (41, 50), "65 row blocks x two chunks: every column planted, the last chunk's too", seed=3120),
]
TIE_CASES = [_case("ds", G0, g1, f"cross-chunk tie, {what}", tie=v)
             for g1 in ((41, 50), (50, 82), (25, 41), (17, 121))
             for v, what in (("a", "first maximum wins: the chunk merge keeps the earlier index and adds the counts"),
                             ("b", "first maximum in the border: the re-scan walks into the later chunk"))]
SKH_CASES = [
    _case("skh", G0, (31, 33), "S + 1 = 1024 fills the last 64-column block of skh_cols_kernel exactly"),
    _case("skh", G0, (25, 41), "chunked skh_conf_kernel: second chunk of 1 column"),
    _case("skh", G0, (27, 38), "chunked skh_conf_kernel: second chunk of 2 columns, even S"),
    _case("skh", G0, (17, 121), "chunked skh_conf_kernel: three chunks"),
    _case("skh", (1, 7), (10, 13), "L = 7: fewer rows than the 16 waves of the column step", border=0),
    _case("skh", (41, 50), G0, "65 row blocks: L + 1 = 2051 rows in the row step"),
    # prefilter off: a row's unit of mass split over two identical columns leaves each 0.47 and each column's dustbin 0.53, so
    # with the prefilter both columns are zeroed and no tie is left to resolve
    _case("skh", G0, (17, 121), "cross-chunk tie, first maximum in the border: the re-scan reads the published matrix", tie="b",
          prefilter=False),
]
DS_CASES = COLUMN_CASES + ROW_CASES + MANY_ROW_CASES + TIE_CASES
ALL_CASES = DS_CASES + SKH_CASES
for _i, _c in enumerate(ALL_CASES):
    if _c["seed"] is None:
        _c["seed"] = 1000 + _i
BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES)


def case_id(c):
    return c["id"]


def find(kind, S=None, L=None, tie=None):
    hits = [c for c in ALL_CASES if c["kind"] == kind and c["tie"] == tie and (S is None or c["S"] == S) and (L is None or c["L"] == L)]
    assert hits, (kind, S, L, tie)
    return hits[0]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _interior(hw, border):
    """bool [h * w]: cells outside the border frame."""
    m = torch.zeros(hw, dtype=torch.bool)
    m[border:hw[0] - border, border:hw[1] - border] = True
    return m.flatten()


def _inputs(c):
    """(f0 [n, L, C], f1 [n, S, C] fp32, planted [n, K, 2] (row, column), noise, generator)."""
    g = torch.Generator().manual_seed(c["seed"])
    L, S = c["L"], c["S"]
    if c["kind"] == "ds":
        ch, noise, k = C_DS, 0.1, min(L, S)
    else:                       # the recipe of pope_amd.synth.sinkhorn_case
        ch, noise, k = C_SKH, 0.3, int(0.6 * min(L, S))
    f0 = torch.randn(N_PAIRS, L, ch, generator=g)
    f1 = torch.randn(N_PAIRS, S, ch, generator=g)
    planted = []
    for b in range(N_PAIRS):
        rows = torch.randperm(L, generator=g)[:k]
        cols = torch.randperm(S, generator=g)[:k]
        f1[b, cols] = f0[b, rows] + noise * torch.randn(k, ch, generator=g)
        planted.append(torch.stack([rows, cols], 1))
    return f0, f1, torch.stack(planted), noise, g


def _plant_tie(c, f0, f1, planted, noise, g):
    """Per pair: (i, j, j2, expected j_id or -1); f1 edited in place."""
    S, chunk, border = c["S"], chunk_of(c["kind"], c["S"]), c["border"]
    in0, in1 = _interior(c["hw0"], border), _interior(c["hw1"], border)
    col = torch.arange(S)
    ties = []
    for b in range(N_PAIRS):
        rows, cols = planted[b, :, 0], planted[b, :, 1]
        free = torch.ones(S, dtype=torch.bool)
        free[cols] = False
        # the interior planted row with the largest norm: its tied confidence (about half of the untied one) stays clear of thr
        cand = rows[in0[rows]]
        i = int(cand[f0[b, cand].norm(dim=1).argmax()])
        old = int(cols[rows == i])
        where_j = in1 if c["tie"] == "a" else (col // c["hw1"][1] < border)
        j = int((free & where_j & (col < chunk)).nonzero()[0])
        later = free & (col >= chunk)
        j2 = (later & in1).nonzero()
        expect_b = bool(len(j2))
        j2 = int(j2[0]) if expect_b else int(later.nonzero()[-1])      # no interior cell there: a column of the last chunk
        f1[b, old] = torch.randn(f1.shape[2], generator=g)             # row i's first plant is withdrawn
        f1[b, j] = f0[b, i] + noise * torch.randn(f1.shape[2], generator=g)
        f1[b, j2] = f1[b, j]
        assert j // chunk != j2 // chunk
        ties.append((i, j, j2, j if c["tie"] == "a" else (j2 if expect_b else -1)))
    return ties


def _conf(c, f0, f1, ties):
    """The oracle's confidence matrix in the dtype of the inputs, the tie enforced."""
    if c["kind"] == "ds":
        conf = cm.conf_matrix(f0, f1, TEMPERATURE)
    else:
        conf = sinkhorn_cpu.conf_matrix(f0, f1, SKH_BIN_SCORE, SKH_ITERS, c["prefilter"])
    for b, (_, j, j2, _) in enumerate(ties):
        conf[b, :, j2] = conf[b, :, j]
    return conf


def clear_decisions(conf, thr, border, hw0, hw1, merged=()):
    """tests/test_gpu_loftr.py:_clear_decisions for any border (0 included) and any L, S (1 included): (must, may) bool
    [n, L, S].  merged: per pair (column kept, twin column): the twin is left out of the runner-up of its rows."""
    n, L, S = conf.shape
    inside = (_interior(hw0, border)[:, None] & _interior(hw1, border)[None, :])[None].expand(n, -1, -1)
    work = conf
    if merged:
        work = conf.clone()
        for b, (_, twin) in enumerate(merged):
            work[b, :, twin] = 0
    neg = torch.full_like(conf[:, :1, :1], -math.inf)

    def top2(dim):
        if conf.shape[dim] < 2:     # nothing to compete with: the margin is infinite
            return work.max(dim, keepdim=True)[0], neg
        t = work.topk(2, dim=dim).values
        return t.narrow(dim, 0, 1), t.narrow(dim, 1, 1)
    rmax, rsec = top2(2)
    cmax, csec = top2(1)
    must = inside & (work > thr + CLEAR) & (work == rmax) & (work == cmax) & (rmax - rsec > CLEAR) & (cmax - csec > CLEAR)
    may = inside & (work > thr - CLEAR) & (work >= rmax - CLEAR) & (work >= cmax - CLEAR)
    return must, may


def units(got, want):
    """Worst |got - want| in units of the bound ATOL + RTOL |want|."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float(((got - want).abs() / (ATOL + RTOL * want.abs())).max()) if got.numel() else 0.0


def lists_of(c, conf):
    """coarse_match on a confidence matrix, with the per-pair counts dense_match adds."""
    out = cm.coarse_match(conf, c["hw0"], c["hw1"], (8 * c["hw0"][0], 8 * c["hw0"][1]), THR, c["border"])
    out["counts"] = torch.bincount(out["b_ids"], minlength=conf.shape[0]).to(torch.int32)
    return out


_built = {}


def build(c):
    """Inputs and reference of a case, built once and left unchanged: dict(f0, f1 fp32; conf64; ref: the fp64 match list; must,
    may; ties: per pair (i, j, j', expected j_id | -1) or []; oracle_units: the fp32 oracle's own conf_matrix error in units
    of the bound; hw0_i)."""
    if c["id"] in _built:
        return _built[c["id"]]
    f0, f1, planted, noise, g = _inputs(c)
    ties = _plant_tie(c, f0, f1, planted, noise, g) if c["tie"] else []
    if c["kind"] == "skh":
        f0, f1 = (f0 * math.sqrt(12.0)).contiguous(), (f1 * math.sqrt(12.0)).contiguous()
    conf64 = _conf(c, f0.double(), f1.double(), ties)
    merged = [(j, j2) if e == j else (j2, j) for (_, j, j2, e) in ties]
    must, may = clear_decisions(conf64, THR, c["border"], c["hw0"], c["hw1"], merged)
    # the twin that is kept in `work` is the expected one; where neither is expected both lie in the border
    d = dict(case=c, f0=f0, f1=f1, conf64=conf64, ref=lists_of(c, conf64), must=must, may=may, ties=ties,
             hw0_i=(8 * c["hw0"][0], 8 * c["hw0"][1]))
    d["oracle_units"] = units(oracle32(d), conf64)
    _built[c["id"]] = d
    return d


def oracle32(d):
    """The fp32 oracle's confidence matrix of a built case (the tie enforced)."""
    return _conf(d["case"], d["f0"], d["f1"], d["ties"])


def stand_in(d, conf, lists_from=None):
    """What dense_match returns, made from a confidence matrix by the oracle's selection (lists_from: the matrix the selection
    reads, where it is not the published one)."""
    out = lists_of(d["case"], conf if lists_from is None else lists_from)
    out["conf_matrix"] = conf
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def check(d, got, what=""):
    """Hold `got` (a dense_match dict with conf_matrix, or a stand-in) to the fp64 reference of the built case d.  Returns
    (worst error of mconf and conf_matrix in units of the bound, the fp32 oracle's conf_matrix error in the same units)."""
    c, ref, conf64 = d["case"], d["ref"], d["conf64"]
    tag = f"{c['id']} {what}: "
    cpu = {k: got[k].cpu() if torch.is_tensor(got[k]) else got[k] for k in LIST_KEYS + ("mconf", "counts", "conf_matrix")}
    # lists
    for k in ("b_ids", "i_ids", "j_ids"):
        assert cpu[k].dtype == torch.int64 and cpu[k].shape == ref[k].shape and torch.equal(cpu[k], ref[k]), \
            tag + f"{k}: {len(cpu[k])} entries against {len(ref[k])} of the reference" + _first_difference(cpu, ref)
    assert [int(v) for v in cpu["counts"]] == ref["counts"].tolist(), tag + "counts"
    for k in ("mkpts0_c", "mkpts1_c"):
        assert cpu[k].dtype == torch.float32 and torch.equal(cpu[k], ref[k].float()), tag + k
    # decisions
    acc = torch.zeros_like(d["must"])
    acc[cpu["b_ids"], cpu["i_ids"], cpu["j_ids"]] = True
    assert bool((d["may"] | ~acc).all()), tag + "a match the reference clearly rejects was accepted"
    assert bool((acc | ~d["must"]).all()), tag + "a clear reference match is missing"
    # values
    want_m = conf64[ref["b_ids"], ref["i_ids"], ref["j_ids"]]
    e_m = units(cpu["mconf"], want_m)
    assert cpu["mconf"].shape == want_m.shape and e_m <= 1.0, tag + f"mconf is {e_m:.3f} of the bound (rtol {RTOL:g}, atol {ATOL:g})"
    conf = cpu["conf_matrix"]
    assert conf is not None and conf.shape == conf64.shape and bool(conf.isfinite().all()), tag + "conf_matrix"
    e_c = units(conf, conf64)
    if e_c > 1.0:
        bad = ((conf.double() - conf64).abs() / (ATOL + RTOL * conf64.abs()))
        b, i, j = np.unravel_index(int(bad.argmax()), bad.shape)
        raise AssertionError(tag + f"conf_matrix is {e_c:.3f} of the bound at [{b}, {i}, {j}]: {float(conf[b, i, j]):.9g} against "
                             f"{float(conf64[b, i, j]):.9g}; {int((bad > 1).sum())} entries beyond it, columns "
                             f"{sorted(set((bad > 1).nonzero()[:, 2].tolist()))[:8]}")
    return max(e_m, e_c), d["oracle_units"]


def _first_difference(cpu, ref):
    a = list(zip(cpu["b_ids"].tolist(), cpu["i_ids"].tolist(), cpu["j_ids"].tolist()))
    b = list(zip(ref["b_ids"].tolist(), ref["i_ids"].tolist(), ref["j_ids"].tolist()))
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"; first difference at {k}: got (b, i, j) = {x}, reference {y}"
    return f"; the shorter list is a prefix of the longer (next: {(a + b)[min(len(a), len(b))] if a != b else None})"


def expected_ties(d):
    """[(pair, i, j, j', expected j_id | -1)] of a tie case."""
    return [(b, *t) for b, t in enumerate(d["ties"])]


def check_ties(d, got):
    """The tie rows of `got`: the expected j_id (or no match), and, when conf_matrix is published, bit-equal twin columns."""
    b_ids, i_ids, j_ids = got["b_ids"].cpu(), got["i_ids"].cpu(), got["j_ids"].cpu()
    for b, i, j, j2, e in expected_ties(d):
        hit = ((b_ids == b) & (i_ids == i)).nonzero().flatten()
        if e < 0:
            assert len(hit) == 0, f"{d['case']['id']}: pair {b} row {i} has both maxima in the border, got j_id {j_ids[hit].tolist()}"
        else:
            assert len(hit) == 1 and int(j_ids[hit[0]]) == e, \
                f"{d['case']['id']}: pair {b} row {i} ties columns {j} and {j2}: expected j_id {e}, got {j_ids[hit].tolist()}"
        conf = got.get("conf_matrix")
        if conf is not None:
            assert torch.equal(conf[b, :, j], conf[b, :, j2]), f"{d['case']['id']}: pair {b}: identical columns {j}, {j2} differ in conf_matrix"
            assert float(conf[b, i, j]) == float(conf[b, i].max()), f"{d['case']['id']}: pair {b}: the tied value is not row {i}'s maximum"
