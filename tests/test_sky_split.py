"""CPU: the skyline-aware split and order rules of the throughput list (psoap_amd/csrc/dag_plan.hpp, PSOAP_SKY_SPLIT) and the
host replay of a launch (tools/dag_replay.py).  Under PSOAP_SKY_SPLIT=0 the list is the one the planner built before the
rules (sha256 digests recorded at that commit, tests/golden/sky_split_parent_v1.json); a dense list never changes; every new
list is complete, its PART ranges partition the clipped update, its waits name smaller tickets; the happens-before
checker of tests/protocol_model.py, with the kernel's scheme-0 events inside a skyline, finds no unordered pair."""
import json
import os
from collections import defaultdict

import numpy as np
import pytest

import protocol_model as pm
import sky_split_cases as cases
from sky_split_cases import WORKERS, dag_replay
from test_sky_plan import CTR_MASK, DIAG, FUSED, NOSOLVE, OFF, PART, TYPE_MASK, plan_dense, plan_sky

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sky_split_parent_v1.json")))
KEYS = sorted(GOLDEN)


@pytest.fixture(autouse=True)
def default_rules(monkeypatch):
    for name in ("PSOAP_SKY_SPLIT", "PSOAP_DAG_SPLIT_PCT", "PSOAP_DAG_SPLIT_MIN", "PSOAP_DAG_SCHEME"):
        monkeypatch.delenv(name, raising=False)


def test_the_cases_are_the_recorded_ones():
    got = {key: (B, P, first) for key, B, P, first in cases.list_cases()}
    assert sorted(got) == KEYS
    for key in KEYS:
        assert got[key] == (GOLDEN[key]["B"], GOLDEN[key]["P"], GOLDEN[key]["first"]), key
    assert any(GOLDEN[key]["first"] != [0] * GOLDEN[key]["P"] for key in KEYS)


@pytest.mark.parametrize("key", KEYS)
def test_the_switch_gives_the_parents_list(key, monkeypatch):
    g = GOLDEN[key]
    monkeypatch.setenv("PSOAP_SKY_SPLIT", "0")
    assert cases.digest(plan_sky(g["B"], g["P"], g["first"], WORKERS)) == g["sky"]


@pytest.mark.parametrize("key", KEYS)
def test_a_dense_list_is_unchanged(key):
    g = GOLDEN[key]
    dense = plan_dense(g["B"], g["P"], WORKERS)
    zero = plan_sky(g["B"], g["P"], [0] * g["P"], WORKERS)
    assert cases.digest(dense) == g["dense"]
    assert dense[0].tobytes() == zero[0].tobytes() and dense[1:] == zero[1:]


@pytest.mark.parametrize("key", KEYS)
def test_every_new_list_is_well_formed(key):
    g = GOLDEN[key]
    B, P, first = g["B"], g["P"], g["first"]
    tasks, n_slots, n_ctrs, qf = plan_sky(B, P, first, WORKERS)
    if not any(first):                           # (length scales x 4: the dense list, test_a_dense_list_is_unchanged)
        assert cases.digest((tasks, n_slots, n_ctrs, qf)) == g["dense"]
        return
    ty = tasks["type"] & TYPE_MASK
    flags = tasks["type"]
    queue = np.zeros(len(tasks), dtype=int)
    for gq in range(8):
        queue[qf[gq]:qf[gq + 1]] = gq
    row_tiles = [sum(1 for j in range(q, P) if first[j] <= q) for q in range(P)]
    finals, parts = {}, defaultdict(list)
    slots = set()
    for t, k in enumerate(tasks):
        b, q, j = int(k["b"]), int(k["q"]), int(k["j"])
        assert b < B and first[j] <= q <= j < P
        if ty[t] == PART:
            assert k["slot"] < n_slots and int(k["slot"]) not in slots and k["ctr"] < n_ctrs and k["pb"] > k["pa"]
            slots.add(int(k["slot"]))
            parts[(b, q, j)].append(t)
        else:
            assert ty[t] in (DIAG, OFF) and (b, q, j) not in finals      # each tile inside the envelope final exactly once
            finals[(b, q, j)] = t
            assert int(k["ctr"]) >> 24 == (P - q) - row_tiles[q], "the row's shortfall against the dense P - q"
            assert (int(k["ctr"]) & CTR_MASK) < max(n_ctrs, 1)
    assert set(finals) == {(b, q, j) for b in range(B) for j in range(P) for q in range(first[j], j + 1)}
    ctr_users = defaultdict(set)
    for (b, q, j), t in finals.items():
        ps = parts.get((b, q, j), [])
        assert int(tasks["S"][t]) == len(ps) + 1
        pos = first[j]
        for p in ps + [t]:                       # the ranges tile [first[j], q) without gap or overlap
            assert int(tasks["pa"][p]) == pos and queue[p] == queue[t]
            pos = int(tasks["pb"][p])
        assert pos == q
        if ps:
            ctr = int(tasks["ctr"][t]) & CTR_MASK
            ctr_users[ctr].add((b, q, j))
            assert all(int(tasks["ctr"][p]) == ctr for p in ps)
            assert [int(tasks["slot"][p]) for p in ps] == list(range(int(tasks["slot"][t]), int(tasks["slot"][t]) + len(ps)))
    assert all(len(v) == 1 for v in ctr_users.values()), "one counter per split tile"
    assert set(parts) <= set(finals)
    # every wait names a smaller ticket (of the same queue: a matrix lives in one queue)
    row_last = defaultdict(lambda: -1)
    for (b, q, j), t in finals.items():
        row_last[(b, q)] = max(row_last[(b, q)], t)
    for t, k in enumerate(tasks):
        b, q, j = int(k["b"]), int(k["q"]), int(k["j"])
        for m in range(int(k["pa"]), int(k["pb"])):                      # the operands of the update
            assert finals[(b, m, q)] < t and finals[(b, m, j)] < t
        if ty[t] == PART:
            continue
        assert all(p < t for p in parts.get((b, q, j), []))              # the partial tiles it gathers
        if q > first[j]:
            assert finals[(b, q - 1, j)] < t                             # its turn at the right-hand side block j
        if ty[t] == OFF:
            assert finals[(b, q, q)] < t                                 # potrf(q)
            assert bool(flags[t] & FUSED) == (j == q + 1)
        elif q >= 1:
            assert flags[t] & NOSOLVE and finals[(b, q - 1, q)] == t - 1 and flags[t - 1] & FUSED   # continues the strip solve
            assert all(row_last[(b, m)] < t for m in range(q - 2))       # rows_done >= q - 2


# ---- the happens-before check inside a skyline ----------------------------------------------------------------------
class SkyModel(pm.Model01):
    """Model01's scheme 0 on ONE matrix's tasks of a skyline list: the events of the kernel's generic path with tile-level
    dependencies, a block row counted against its tiles inside the envelope (the shortfall the finals' records carry), and a
    right-hand side block j that is touched by the rows first[j] .. j only."""

    def __init__(self, tasks, P, first, b):
        self.scheme, self.first = 0, first
        self.P, self.inorder, self.acc_chain, self.rv_wait = P, True, False, True
        self.g = pm.Graph()
        self.tasks = tasks[tasks["b"] == b]
        self.flags = self.tasks["type"].copy()
        self.kind = self.tasks["type"] & pm.TYPE_MASK
        self.pubs, self.adds, self.waits = defaultdict(list), defaultdict(list), []
        self.writes, self.reads, self.last = defaultdict(dict), [], {}
        self.launch = self.g.node("launch")
        self.build_sky()

    def build_sky(self):
        P, tasks, first = self.P, self.tasks, self.first
        row_members = defaultdict(list)
        prev_end = None
        rvv = lambda j, q: q - first[j]          # writes to right-hand side block j before row q's (q >= first[j])
        for t, k in enumerate(tasks):
            q, j, S, pa, pb = int(k["q"]), int(k["j"]), int(k["S"]), int(k["pa"]), int(k["pb"])
            ctr, slot, f = int(k["ctr"]) & CTR_MASK, int(k["slot"]), int(self.flags[t])
            assert not f & pm.CHAIN
            wt, wt_v = ("wt", q % 3), q // 3
            if self.kind[t] == pm.PART:
                s = self.Seq(self, t, f"PART({q},{j})#{slot}")
                self.update(s, q, j, pa, pb)
                s.write(("gslot", slot), 0)
                s.add(("arrive", ctr))
                self.last[t] = prev_end = s.cur
                continue

            def gather(s):
                if S > 1:
                    s.wait(("arrive", ctr), S - 1, counter=True)
                    for u in range(S - 1):
                        s.read(("gslot", slot + u), 0)

            if self.kind[t] == pm.DIAG:
                s = self.Seq(self, t, f"DIAG({q})")
                if f & pm.NOSOLVE:               # owned: run right behind the strip solve of tile (q - 1, q), by its workgroup
                    assert prev_end is not None and int(tasks[t - 1]["q"]) == q - 1 and int(tasks[t - 1]["j"]) == q
                    self.g.edge(prev_end, s.cur)
                self.update(s, q, q, pa, pb)
                gather(s)
                s.write(("tile", q, q), 0)
                s.wait("rows_done", q - 2 if q >= 3 else 0)
                s.read(("tile", q, q), 0)
                s.read(("rv", q), rvv(q, q))
                s.write(("tile", q, q), 1)
                s.write(wt, wt_v)
                s.write(("rv", q), rvv(q, q) + 1)
                s.write(("acc", q), 0)
                if q > 0:
                    s.wait("potrf_done", q)
                s.publish("potrf_done", q + 1)
            else:
                s = self.Seq(self, t, f"OFF({q},{j})")
                self.update(s, q, j, pa, pb)
                gather(s)
                s.write(("tile", q, j), 0)
                s.wait("potrf_done", q + 1)
                s.read(wt, wt_v)
                s.read(("tile", q, j), 0)
                s.read(("rv", q), rvv(q, q) + 1)
                s.write(("tile", q, j), 1)
                s.read(("rv", j), rvv(j, q))
                s.write(("rv", j), rvv(j, q) + 1)
            self.last[t] = s.cur
            row_members[q].append(t)
            if self.kind[t] == pm.OFF:
                s.publish(("rvrow", j), q + 1)               # (behind the row's count: see k_chol_dag)
            prev_end = s.cur
        g = self.g
        for q in range(P):
            members = [self.last[t] for t in row_members[q]]
            assert len(members) == sum(1 for j in range(q, P) if first[j] <= q)
            assert all(int(tasks["ctr"][t]) >> 24 == (P - q) - len(members) for t in row_members[q])
            n = g.node(f"rows_done={q + 1}")
            for mbr in members:
                g.edge(mbr, n)
            if q > 0:
                g.edge(self.pubs["rows_done"][-1][1], n)
            self.pubs["rows_done"].append((q + 1, n))
        rep = g.node("report")
        for ev in self.last.values():
            g.edge(ev, rep)
        for q in range(P):
            self.reads.append((("acc", q), 0, rep, "report"))
        self.wait_nodes = []
        for flag, target, ev, counter in self.waits:
            cands = self.adds[flag] if counter else [e for v, e in self.pubs[flag] if v >= target]
            assert len(cands) >= (target if counter else 1), f"nobody ever brings {flag} to {target}"
            n = g.node(f"{flag}>={target}")
            g.edge(n, ev)
            self.wait_nodes.append([n, ev, set(cands), target if counter else 0])
        self.refine()


# (the headline list, 966 tasks per matrix, takes this checker nine minutes: it gets the ticket-order checks above, and the
# same rules are checked here at the sizes where they start to act)
@pytest.mark.parametrize("key", [k for k in KEYS if any(GOLDEN[k]["first"]) and GOLDEN[k]["P"] <= 16])
def test_the_new_lists_are_ordered_by_hand_offs_alone(key):
    g = GOLDEN[key]
    tasks = plan_sky(g["B"], g["P"], g["first"], WORKERS)[0]
    # a matrix of the first queue and one of the last; the band at P = 16, where a diagonal tile's history comes in two parts
    # and strips in up to eight pieces, takes 8 s per matrix: one
    for b in ((0, g["B"] - 1) if g["P"] <= 10 else (g["B"] - 1,)):
        assert SkyModel(tasks, g["P"], g["first"], b).races() == []


def test_the_band_the_checker_sees_uses_both_kinds_of_split():
    g = GOLDEN["mid_band"]
    tasks = plan_sky(g["B"], g["P"], g["first"], WORKERS)[0]
    fin = tasks[(tasks["type"] & TYPE_MASK) != PART]
    assert fin["S"][fin["q"] == fin["j"]].max() == 3 and fin["S"][fin["q"] != fin["j"]].max() == 8


def test_the_headline_list_uses_the_new_rules():
    """what the checker above sees on the headline list: pre-accumulations in several parts, strips in several pieces, and
    the tiles of a block row column by column over the four matrices of a queue"""
    g = GOLDEN["headline"]
    tasks, _, _, qf = plan_sky(g["B"], g["P"], g["first"], WORKERS)
    ty = tasks["type"] & TYPE_MASK
    fin = tasks[ty != PART]
    assert fin["S"][fin["q"] == fin["j"]].max() == 4 and fin["S"][fin["q"] != fin["j"]].max() == 8
    q0 = tasks[qf[0]:qf[1]]
    row = q0[((q0["type"] & TYPE_MASK) == OFF) & (q0["q"] == 20)]
    assert [int(b) for b in row["b"][:8]] == [0, 8, 16, 24, 0, 8, 16, 24] and [int(j) for j in row["j"][:8]] == [21] * 4 + [22] * 4


def test_the_sky_model_notices_a_wait_that_is_taken_away(monkeypatch):
    """the clean result is not vacuous: without the strip solves' wait for the factorisation the pair shows up"""
    g = GOLDEN["narrow_odd_1250"]
    tasks = plan_sky(g["B"], g["P"], g["first"], WORKERS)[0]
    orig = pm.Model.Seq.wait

    def wait(self, flag, target, counter=False):
        if flag == "potrf_done" and "OFF" in self.label:
            return
        return orig(self, flag, target, counter)
    monkeypatch.setattr(pm.Model.Seq, "wait", wait)
    assert SkyModel(tasks, g["P"], g["first"], 0).races()


# ---- the replay -----------------------------------------------------------------------------------------------------
def headline_replay(workers):
    first, first16 = cases.headline()
    tasks, _, _, qf = plan_sky(32, 47, first, workers)
    return dag_replay.Replay(tasks, qf, None, workers, first16).run()


def test_the_replay_is_deterministic_and_starts_nothing_before_its_waits_are_met():
    a, b = headline_replay(WORKERS), headline_replay(WORKERS)
    assert a.span == b.span and np.array_equal(a.start, b.start) and np.array_equal(a.end, b.end)
    assert a.report() == b.report()
    tasks, kind = a.tasks, a.kind
    assert a.checked_waits > len(tasks)
    finals = {(int(k["b"]), int(k["q"]), int(k["j"])): t for t, k in enumerate(tasks) if kind[t] != PART}
    by_ctr = defaultdict(list)
    for t in np.flatnonzero(kind == PART):
        by_ctr[int(tasks["ctr"][t])].append(t)
    c = a.c
    for t, k in enumerate(tasks):
        b_, q, j, pa, pb = int(k["b"]), int(k["q"]), int(k["j"]), int(k["pa"]), int(k["pb"])
        # the last panel's products come behind both operands of row pb - 1; the stores behind every partial tile; the strip
        # solve behind the factorisation: a task's end lies at least the work that follows each wait behind that wait's source
        tail = c["store_part"] if kind[t] == PART else c["store_final"] + (c["potrf"] if kind[t] == DIAG else c["solve"])
        if pb > pa:
            for col in (q, j):
                assert a.end[t] >= a.end[finals[(b_, pb - 1, col)]] + tail - 1e-9
        if kind[t] != PART:
            for p in by_ctr.get(int(k["ctr"]) & CTR_MASK, []) if int(k["S"]) > 1 else []:
                assert a.end[t] >= a.end[p] + tail - 1e-9
        if kind[t] == OFF:
            assert a.end[t] >= a.end[finals[(b_, q, q)]] + c["solve"] - 1e-9
        assert a.end[t] > a.start[t]


def test_one_worker_takes_the_sum_of_the_costs():
    r = headline_replay(1)
    c, kind = r.c, r.kind
    stages = int(r.head.sum() + r.last.sum())
    folds = int((r.tasks["S"][kind != PART].astype(int) - 1).sum())
    want = (c["task"] * len(r.tasks) + c["stage"] * stages + c["fold"] * folds + c["store_part"] * int((kind == PART).sum())
            + c["store_final"] * int((kind != PART).sum()) + c["solve"] * int((kind == OFF).sum()) + c["potrf"] * int((kind == DIAG).sum()))
    assert abs(r.span - want) <= 1e-9 * want
    assert sum(r.waited.values()) == 0.0 and r.tail == 0.0
