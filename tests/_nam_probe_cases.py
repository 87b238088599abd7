"""Probe inputs for MS_PLUGINS_NU_NN_NAM and a model of what they must give,
shared by tests/test_nam_probe_cases.py (CPU: the model against the C oracle,
and what the probes cover) and tests/test_gpu_nam_probes.py (the kernels
against the model). Test infrastructure, never product code.

The mechanism. With score weights (w_nn, w_na) such that 10 w_nn > 100 w_na,
the one feasible row that carries a pod's name digit wins whatever the other
rows score, so the cycle's result IS that row's normalised NodeAffinity score:
node = the row, score = 10 w_nn + w_na F[class][row]. A probe STATE is the
table with every name digit 255 except up to ten target rows carrying the
digits 0..9; its pods are every class (term set id, toleration) times the ten
digits. F does not depend on the digits, so moving the probes is an upsert of
the changed rows.

Raw scores by construction. Node zone and label2 ids lie in 0..3 and read as
one 4-bit mask m = zone | label2 << 2. Every term set has four terms: term t
matches when bit t of m is set (terms 0, 1 on the zone id sets {1, 3}, {2, 3}
with every label2 id allowed, terms 2, 3 the same on label2). A row's raw score
for a class is the subset sum of the class's four weights over m.
"""
from __future__ import annotations

import functools

import numpy as np

import _nam_required_ref as ref
from minisched_amd import _lib

ALL = (1 << 256) - 1
BIT_SETS = ((0b1010, ALL), (0b1100, ALL), (ALL, 0b1010), (ALL, 0b1100))  # (zone ids, label2 ids) of term t
W_PROBE = (11, 1)
MULTI = (3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15)
SEED = 97


# ---- the generator ---------------------------------------------------------
def node_rows(n, seed, head, multi):
    """n node records, no name digit yet: about 8 % mask 0, a fraction `multi`
    of multi-bit masks, the rest single-bit; the first `head` rows mask 0 (the
    anchor comes late); the last four masks 1, 3, 7, 15, schedulable; about
    10 % unschedulable."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    m = np.left_shift(1, rng.integers(0, 4, n))
    m = np.where(u < 0.08, 0, np.where(u < 0.08 + multi, np.asarray(MULTI)[rng.integers(0, len(MULTI), n)], m))
    m[:head] = 0
    m[-4:] = (1, 3, 7, 15)
    uns = rng.random(n) < 0.10
    uns[-4:] = False
    nr = np.zeros(n, dtype=_lib.NODE_REC)
    nr["zone"], nr["label2"] = m & 3, m >> 2
    nr["unschedulable"], nr["name_digit"], nr["allowed_pods"] = uns, 255, 110
    return nr


def set_weights(n_any, n_high, n_100, n_34, n_25, n_big, rs, seed):
    """The four weights of every term set, in the issue's class mix: drawn from
    1..100; from 51..100 (every pair rescales); {100, 1, x, y} (raw exactly 100
    and 101); from 1..34 (few rescales, all near 101); from 1..25, or one weight
    spread over 52..94 and three small ones with a total of 100 at the most (no
    rescale at all: F is the raw score, which fills the upper values of F); and
    for each r in rs, k = (r - 1) // 100 hundreds then r - 100 k, so
    the mask of the k + 1 low bits has raw exactly r."""
    rng = np.random.default_rng(seed)
    out = []
    out += [tuple(int(x) for x in rng.integers(1, 101, 4)) for _ in range(n_any)]
    out += [tuple(int(x) for x in rng.integers(51, 101, 4)) for _ in range(n_high)]
    out += [(100, 1, int(rng.integers(1, 101)), int(rng.integers(1, 101))) for _ in range(n_100)]
    out += [tuple(int(x) for x in rng.integers(1, 35, 4)) for _ in range(n_34)]
    out += [tuple(int(x) for x in rng.integers(1, 26, 4)) for _ in range(n_25)]
    for i in range(n_big):
        big = 52 + (42 * i) // max(1, n_big - 1)
        rest = 100 - big  # (6 at the least)
        a = int(rng.integers(1, rest - 1))
        b = int(rng.integers(1, rest - a))
        out.append((big, a, b, int(rng.integers(1, rest - a - b + 1))))
    for r in rs:
        k = (r - 1) // 100
        w = [100] * k + [r - 100 * k]
        out.append(tuple(w + [int(x) for x in rng.integers(1, 101, 4 - len(w))]))
    return out


def term_sets(weights):
    return _lib.nam_term_sets_ext_array([[(w, z, l) for w, (z, l) in zip(ws, BIT_SETS)] for ws in weights])


def required_terms(n_sets, seed):
    """Required sets designed on the same bits: a third none; the rest one or two
    terms (zone id set, label2 id set), each a non-empty subset of the ids 0..3
    or every id."""
    rng = np.random.default_rng(seed)

    def ids():
        return ALL if rng.integers(0, 3) == 0 else int(rng.integers(1, 16))

    return [None if rng.integers(0, 3) == 0 else [(ids(), ids()) for _ in range(int(rng.integers(1, 3)))]
            for _ in range(n_sets)]


class Table:
    """One probe table: node records without digits, the weights of its term
    sets, optional required terms per set, rows that are deleted."""

    def __init__(self, name, nodes, weights, required=None, dead=()):
        self.name, self.nodes, self.weights, self.required = name, nodes, weights, required
        self.dead = tuple(int(d) for d in dead)
        self.n_sets = len(weights)
        self.ts = term_sets(weights)
        self.rq = _lib.nam_required_sets_array(required) if required is not None else None
        # every class: ids 0 (no set) .. n_sets, and one id past the registered sets
        self.classes = [(sid, tol) for sid in range(self.n_sets + 2) for tol in (0, 1)]

    def with_digits(self, targets):
        nr = self.nodes.copy()
        for d, t in enumerate(targets):
            nr["name_digit"][t] = d
        return nr

    def pods(self, salt=0):
        """Every class times the ten digits, classes interleaved in batch order."""
        cls = np.asarray(self.classes, dtype=np.int64)
        sid, tol = np.repeat(cls[:, 0], 10), np.repeat(cls[:, 1], 10)
        dig = np.tile(np.arange(10), len(cls))
        order = np.random.default_rng(SEED + salt).permutation(len(sid))
        pr = np.zeros(len(sid), dtype=_lib.POD_REC)
        pr["ordinal"] = np.arange(len(sid))
        pr["name_digit"], pr["tolerates_unschedulable"] = dig[order], tol[order]
        pr["pref_zone"], pr["pref_weight"] = sid[order] & 0xFF, sid[order] >> 8
        return pr


@functools.lru_cache(maxsize=None)
def table(name):
    if name in ("all_rows", "required"):
        nodes = node_rows(640, 11, head=9, multi=0.02)
        w = set_weights(10, 10, 10, 8, 4, 14, (101, 127, 150, 200, 201, 300, 301, 400), 12)
        return Table(name, nodes, w, required_terms(len(w), 13) if name == "required" else None)
    if name == "shards":
        t = table("all_rows")
        return Table(name, t.nodes, t.weights, dead=(64,))
    if name == "multi_tile":
        # 600 sets: 1,202 classes, for which nam_layout gives 8 row segments of 1,088
        # rows = one LDS tile of 1,024 rows and a second of 64
        nodes = node_rows(8704, 21, head=37, multi=0.012)
        return Table(name, nodes, set_weights(70, 70, 50, 40, 20, 50, range(101, 401), 22))
    raise KeyError(name)


SHARD_CUTS = (0, 64, 65, 300, 640)
MULTI_TILE_CUT = 4133  # (not a multiple of 64)
MULTI_TILE_SEG = 1088


# ---- the model -------------------------------------------------------------
def inloop(raw):
    """RunScorePlugins' in-loop hook for NodeAffinity (DefaultNormalizeScore,
    reverse = false) on one feasible list: the list starts zero-filled; after
    each row's score lands the WHOLE list is rescaled by 100 v // max (later
    entries are 0 and stay 0). A step whose maximum is 100 (or 0: skipped by the
    hook) is the identity and is not carried out."""
    lst = np.zeros(len(raw), dtype=np.int64)
    mx = 0
    for k, r in enumerate(raw):
        lst[k] = r
        mx = max(mx, int(r))
        if mx > 0 and mx != 100:
            lst[:k + 1] = 100 * lst[:k + 1] // mx
            mx = 100
    return lst


class ClassList:
    """One class on one table: its feasible rows in list order, their raw scores,
    F, and the FitError mask of a pod with no feasible row."""

    def __init__(self, rows, raw, F, mask, n):
        self.rows, self.raw, self.F, self.mask = rows, raw, F, mask
        self.at = np.full(n, -1, dtype=np.int64)
        self.at[rows] = np.arange(len(rows))


@functools.lru_cache(maxsize=None)
def model(name):
    """{(effective set id, toleration): ClassList} of a table."""
    t = table(name)
    nr = t.nodes
    present = nr["allowed_pods"] >= 0
    present[np.asarray(t.dead, dtype=np.int64)] = False
    uns = nr["unschedulable"] != 0
    m = nr["zone"].astype(np.int64) | nr["label2"].astype(np.int64) << 2
    zl = [(z, l) for z, l in zip(nr["zone"].tolist(), nr["label2"].tolist())]
    out = {}
    for sid in range(t.n_sets + 1):
        ws = t.weights[sid - 1] if sid else (0, 0, 0, 0)
        sums = np.asarray([sum(w for b, w in enumerate(ws) if s >> b & 1) for s in range(16)], dtype=np.int64)
        terms = t.required[sid - 1] if (sid and t.required is not None) else None
        ok = np.asarray([ref.passes(terms, z, l) for z, l in zl], dtype=bool)
        for tol in (0, 1):
            pass_nu = present & (~uns | bool(tol))
            rows = np.nonzero(pass_nu & ok)[0]
            raw = sums[m[rows]]
            mask = (1 if (present & ~pass_nu).any() else 0) | (8 if (pass_nu & ~ok).any() else 0)
            out[(sid, tol)] = ClassList(rows, raw, inloop(raw), mask, len(nr))
    return out


def class_of(t, sid, tol):
    return (sid if sid <= t.n_sets else 0, int(tol))


def expect(name, targets, pods, weights=W_PROBE, seed=SEED, node_base=0):
    """What the cycle must give for the probe pods of a state: node, code, score,
    mask, and `hit` (the pod's target row is feasible for its class, so the
    result is the probe itself; else selectHost over w_na F by the r3 key)."""
    t, M = table(name), model(name)
    w_nn, w_na = weights
    assert 10 * w_nn > 100 * w_na and 10 * w_nn + 100 * w_na < 2048
    n = len(pods)
    o = dict(node=np.full(n, -1, np.int32), score=np.zeros(n, np.int64), code=np.zeros(n, np.int32),
             mask=np.zeros(n, np.uint32), hit=np.zeros(n, bool))
    keys = list(M)
    index = {k: i for i, k in enumerate(keys)}
    # F of every class at the ten targets (-1: infeasible for the class, or no such target)
    at = np.full((len(keys), 10), -1, dtype=np.int64)
    for i, k in enumerate(keys):
        c = M[k]
        for d, r in enumerate(targets):
            if c.at[r] >= 0:
                at[i, d] = c.F[c.at[r]]
    sid = ref.set_id(pods)
    ci = np.asarray([index[class_of(t, int(s), int(tl))] for s, tl in zip(sid, pods["tolerates_unschedulable"])])
    dig = pods["name_digit"].astype(np.int64)
    f = at[ci, dig]
    hit = f >= 0
    tg = np.asarray(list(targets) + [0] * (10 - len(targets)), dtype=np.int64)
    o["hit"] = hit
    o["node"][hit] = node_base + tg[dig[hit]]
    o["score"][hit] = 10 * w_nn + w_na * f[hit]
    for j in np.nonzero(~hit)[0]:
        c = M[keys[ci[j]]]
        if len(c.rows) == 0:
            o["code"][j], o["mask"][j] = 2, c.mask
        else:
            best = int(ref.keys_r3(seed, pods["ordinal"][j], node_base + c.rows, w_na * c.F).max())
            o["node"][j], o["score"][j] = 0xFFFFF - (best & 0xFFFFF), best >> 52
    return o


def describe(name, targets, pods, j, got_score, weights=W_PROBE):
    """Class, row, raw, expected and received F of probe pod j (for a failure message)."""
    t, M = table(name), model(name)
    sid, tol, d = int(ref.set_id(pods)[j]), int(pods["tolerates_unschedulable"][j]), int(pods["name_digit"][j])
    c = M[class_of(t, sid, tol)]
    row = targets[d] if d < len(targets) else None
    k = int(c.at[row]) if row is not None else -1
    return dict(set=sid, tol=tol, weights=t.weights[sid - 1] if 1 <= sid <= t.n_sets else None, row=row,
                raw=int(c.raw[k]) if k >= 0 else None, want_F=int(c.F[k]) if k >= 0 else None,
                got_F=(int(got_score) - 10 * weights[0]) / weights[1])


# ---- the states ------------------------------------------------------------
def _deal(rows, uns, n_states):
    """Rows dealt round-robin into n_states target lists of at most ten, the
    unschedulable ones first so that no state takes many of them."""
    rows = sorted(set(int(r) for r in rows), key=lambda r: (not uns[r], r))
    assert len(rows) <= 10 * n_states
    return [rows[s::n_states] for s in range(n_states)]


def anchors(name, limit):
    """The anchors (first feasible row of non-zero raw score) of a table's classes
    and the rows next to them, `limit` distinct anchors at the most."""
    seen = []
    for c in model(name).values():
        nz = np.nonzero(c.raw > 0)[0]
        if len(nz) and int(c.rows[nz[0]]) not in seen:
            seen.append(int(c.rows[nz[0]]))
    n = len(table(name).nodes)
    return sorted({r + d for r in sorted(seen)[:limit] for d in (-1, 0, 1) if 0 <= r + d < n})


@functools.lru_cache(maxsize=None)
def states(name):
    """The target lists of a table's probe states."""
    if name == "all_rows":
        return [[s + 64 * d for d in range(10)] for s in range(64)]  # every row once
    if name == "multi_tile":
        t, M = table(name), model(name)
        n, uns = len(t.nodes), t.nodes["unschedulable"] != 0
        rows = [r0 + d for r0 in range(0, n, MULTI_TILE_SEG) for d in (0, 1, 1023, 1024, 1087)]
        rows += [int(M[(0, 0)].rows[0]), int(M[(0, 1)].rows[0])]  # the first feasible row
        rows += anchors(name, 4) + list(range(n - 40, n))
        rest = np.setdiff1d(np.arange(n), rows)
        k = 120 - len(set(rows))
        rows += np.random.default_rng(23).choice(rest, size=k, replace=False).tolist()
        return _deal(rows, uns, 12)
    if name == "shards":
        rows = [0, 1, 62, 63, 65, 66, 298, 299, 300, 301, 638, 639] + anchors("shards", 6) + list(range(620, 640))
        rows = [r for r in rows if r not in table(name).dead]
        st = _deal(rows, table(name).nodes["unschedulable"] != 0, 9)
        return st + [[64 * d + 33 for d in range(10)]]
    a = states("all_rows")
    if name == "host_chunks":
        return [a[0], a[37], a[63]]
    if name == "required":
        return a[::7]
    if name == "w23_2":
        return [a[1], a[15], a[31], a[46], a[63]]
    raise KeyError(name)


def multi_tile_shard_states():
    st = states("multi_tile")
    near = [MULTI_TILE_CUT + d for d in (-2, -1, 0, 1)]
    return [near + [r for r in st[0] if r not in near][:6], st[7]]


def base_table(name):
    """The table a family member's states run on."""
    return name if name in ("all_rows", "multi_tile", "shards", "required") else "all_rows"


# ---- coverage, on the model alone --------------------------------------------
def probed_F(name, state_list=None):
    """(class key, row, raw, F) of every probe of a table's states whose target is
    feasible for the class."""
    M = model(base_table(name))
    out = []
    for targets in (states(name) if state_list is None else state_list):
        for key, c in M.items():
            for r in targets:
                k = int(c.at[r])
                if k >= 0:
                    out.append((key, r, int(c.raw[k]), int(c.F[k])))
    return out


def class_facts(name):
    """Per class of a table: the raw scores that rescale effectively (a feasible
    row with raw r > 100 whose own F is above 0), whether no row rescales, whether
    the table is all zero before the list ends (a row of raw >= 100 with F 0),
    whether raw 100 / 101 occur, and the anchor (row, raw, F, F as a non-anchor)."""
    facts = {}
    for key, c in model(name).items():
        nz = np.nonzero(c.raw > 0)[0]
        anchor = None
        if len(nz):
            k = int(nz[0])
            alt = inloop(np.concatenate(([1], c.raw)))[1:]  # an earlier non-zero row takes the anchor's place
            anchor = (int(c.rows[k]), int(c.raw[k]), int(c.F[k]), int(alt[k]))
        facts[key] = dict(effective=set(c.raw[(c.raw > 100) & (c.F > 0)].tolist()),
                          no_rescale=bool(len(c.raw) and c.raw.max() <= 100),
                          dies=bool(((c.raw >= 100) & (c.F == 0)).any()),
                          raw100=bool((c.raw == 100).any()), raw101=bool((c.raw == 101).any()), anchor=anchor)
    return facts
