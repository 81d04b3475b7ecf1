#!/usr/bin/env python3
"""Writes tests/golden/ransac_host_pins.txt: the cases of tests/test_ransac_host_pins.py and, under each, what
tests/cpp/ransac_host_pins.cpp printed for it.

The committed fixture was generated against the csrc of the parent of the commit that introduced csrc/ransac_host.h, that is
against sim3_host.h, pnp_host.h and initializer_host.h while each still carried its own offsets check, set predicate, layout
loop and selection without replacement:

    git archive <parent> | tar -x -C /tmp/parent
    python tools/gen_ransac_host_pins.py --csrc /tmp/parent/orb_slam2_annotate_amd/csrc

The test then holds every later form of those headers to that text.  Without --csrc it pins whatever the checkout computes:
do that only on a commit whose results are the wanted ones.
"""
import argparse
import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "ransac_host_pins.txt"
SOLVERS = {"sim3": 3, "pnp": 4, "init": 8}                  # the size S of the minimal set
PER_OWNER = {"sim3": 8, "pnp": 4, "init": 9}                # cam1 cam2 | cam | T1 T2 sigma
N_POINTERS = {"sim3": 14, "pnp": 12, "init": 14}


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


class Call:
    """One call of a solver: K owners with n[k] entries and sets[k] = the minimal sets of owner k."""

    def __init__(self, solver, n, sets):
        self.solver, self.S = solver, SOLVERS[solver]
        self.K, self.N, self.H = len(n), sum(n), sum(len(s) for s in sets)
        self.mask = 0
        self.poff = [0] + list(np.cumsum(n, dtype=np.int64)) if n else [0]
        self.hoff = [0] + list(np.cumsum([len(s) for s in sets], dtype=np.int64)) if n else [0]
        self.sets = [i for owner in sets for s in owner for i in s]
        # written as runs when every owner's sets are one (first_sets) and there are many; what a case edits is a patch
        self.runs = [o.run for o in sets if len(o)] if all(isinstance(o, Run) or not len(o) for o in sets) else None
        self.unedited = list(self.sets)
        K = self.K
        if solver == "sim3":    # cam1 [4K], cam2 [4K]
            self.f = [500.0 + k for k in range(K) for _ in range(4)] + [400.0 + k for k in range(K) for _ in range(4)]
        elif solver == "pnp":   # cam [4K]
            self.f = [500.0 + k + 0.25 * i for k in range(K) for i in range(4)]
        else:                   # T1 [4K], T2 [4K], sigma [K]
            self.f = [0.5 + k + i for k in range(K) for i in range(4)] + [0.25 + k + i for k in range(K) for i in range(4)] + [1.0 + 0.5 * k for k in range(K)]

    def line(self, fn, name):
        sets = [len(self.sets), *self.sets]
        if self.runs is not None and len(self.sets) > 64:
            patches = [(i, x) for i, (x, was) in enumerate(zip(self.sets, self.unedited)) if x != was]
            sets = [-1, len(self.runs), *[x for r in self.runs for x in r], len(patches), *[x for q in patches for x in q]]
        v = [self.K, self.N, self.H, self.mask, len(self.poff), *self.poff, len(self.hoff), *self.hoff, *sets,
             len(self.f), *[fbits(x) for x in self.f]]
        return f"case {self.solver}_{fn} {name} " + " ".join(str(int(x)) for x in v)


class Run(list):
    """the sets of first_sets, which remember (n, count, start)"""


def first_sets(S, n, count, start=0):
    """count distinct-index sets of S out of n, each a run of consecutive indices"""
    r = Run([(start + h + i) % n for i in range(S)] for h in range(count))
    r.run = (n, count, start)
    return r


def base(solver):
    """two owners: 33 entries with 2 sets, S + 2 entries with 1 set"""
    S = SOLVERS[solver]
    return Call(solver, [33, S + 2], [first_sets(S, 33, 2), first_sets(S, S + 2, 1, 1)])


def check_cases(solver):
    S = SOLVERS[solver]
    out = []

    def add(name, edit=None, call=None):
        c = call or base(solver)
        if edit:
            edit(c)
        out.append(c.line("check", name))

    # ---- every refusal, once
    add("k_negative", lambda c: (setattr(c, "K", -1), setattr(c, "f", [])))
    add("k_4097", lambda c: (setattr(c, "K", 4097), setattr(c, "f", [])))
    add("n_negative", lambda c: setattr(c, "N", -1))
    add("h_negative", lambda c: setattr(c, "H", -1))
    if solver == "init":
        add("h_above_2_24", lambda c: setattr(c, "H", (1 << 24) + 1))
    for b in range(N_POINTERS[solver]):
        add(f"null_pointer_{b}", lambda c, b=b: setattr(c, "mask", 1 << b))
    add("pair_off_not_from_0", lambda c: c.poff.__setitem__(0, 1))
    add("pair_off_not_to_total", lambda c: setattr(c, "N", c.N + 1))
    add("pair_off_descends", lambda c: c.poff.__setitem__(1, c.N + 1))
    add("hyp_off_not_from_0", lambda c: c.hoff.__setitem__(0, 1))
    add("hyp_off_not_to_total", lambda c: setattr(c, "H", c.H + 1))
    add("hyp_off_descends", lambda c: c.hoff.__setitem__(1, c.H + 1))
    for what, v in (("nan", float("nan")), ("inf", float("inf"))):
        for at in (0, PER_OWNER[solver] + 1):  # owner 0's first value; one of owner 1, or of the second array
            add(f"owner_value_{what}_at_{at}", lambda c, at=at, v=v: c.f.__setitem__(at, v))
    if solver == "init":
        for what, v in (("zero", 0.0), ("negative", -1.0), ("nan", float("nan")), ("inf", float("inf"))):
            add(f"sigma_{what}", lambda c, v=v: c.f.__setitem__(len(c.f) - 1, v))
    add("too_few_entries_with_sets", call=Call(solver, [33, S - 1], [first_sets(S, 33, 1), [list(range(S))]]))
    for i in range(S):
        add(f"index_negative_at_{i}", lambda c, i=i: c.sets.__setitem__(i, -1))
        add(f"index_n_at_{i}", lambda c, i=i: c.sets.__setitem__(2 * S + i, S + 2))  # owner 1 has S + 2 entries
    for i in range(1, S):
        add(f"index_{i}_repeats_0", lambda c, i=i: c.sets.__setitem__(i, c.sets[0]))
    add("last_repeats_the_one_before", lambda c: c.sets.__setitem__(S - 1, c.sets[S - 2]))
    # 2^26 entries are 2^21 words a mask; 1024 (512 for the Initializer's two masks a set) make 2^31
    big = 1 << 26
    many = 1024 if solver != "init" else 512
    add("mask_words_2_31", call=Call(solver, [big], [first_sets(S, big, many)]))
    add("mask_words_2_31_less_one_mask", call=Call(solver, [big], [first_sets(S, big, many - 1)]))  # accepted
    # ---- two faults in one call: which one is named
    add("two_nan_owner0_repeat_owner1", lambda c: (c.f.__setitem__(1, float("nan")), c.sets.__setitem__(2 * S + 1, c.sets[2 * S])))
    add("two_repeat_owner0_nan_owner1", lambda c: (c.sets.__setitem__(1, c.sets[0]), c.f.__setitem__(4, float("nan"))))
    add("two_bad_set_owner0_too_few_owner1", lambda c: c.sets.__setitem__(0, 40),
        call=Call(solver, [33, S - 1], [first_sets(S, 33, 1), [list(range(S))]]))
    add("two_too_few_owner0_bad_set_owner1", lambda c: c.sets.__setitem__(S, -1),
        call=Call(solver, [S - 1, 33], [[list(range(S))], first_sets(S, 33, 1)]))
    add("two_outside_owner0_repeat_owner1", lambda c: (c.sets.__setitem__(S - 1, 33), c.sets.__setitem__(2 * S + 1, c.sets[2 * S])))
    add("two_in_one_set_repeat_then_outside", lambda c: (c.sets.__setitem__(1, c.sets[0]), c.sets.__setitem__(2, -1)))
    add("two_in_one_set_outside_then_repeat", lambda c: (c.sets.__setitem__(0, -1), c.sets.__setitem__(2, c.sets[1])))
    add("two_null_camera_and_bad_offsets", lambda c: (setattr(c, "mask", 1 << (5 if solver == "sim3" else 4 if solver == "pnp" else 2)),
                                                     c.poff.__setitem__(0, 1)))
    add("two_hyp_off_bad_and_index_outside", lambda c: (c.hoff.__setitem__(0, 1), c.sets.__setitem__(0, -1)))
    add("two_mask_words_and_bad_set_later", lambda c: c.sets.__setitem__(S * many, -1),
        call=Call(solver, [big, S], [first_sets(S, big, many), first_sets(S, S, 1)]))
    # ---- accepted
    add("fine_base")
    add("fine_k0", call=Call(solver, [], []))
    add("fine_owner_without_sets", call=Call(solver, [33, 2, S], [first_sets(S, 33, 1), [], first_sets(S, S, 1)]))
    add("fine_owner_without_entries", call=Call(solver, [0, S], [[], first_sets(S, S, 2)]))
    for n in (S, 32, 33, 64):
        add(f"fine_n{n}", call=Call(solver, [n], [first_sets(S, n, 3)]))
    return out


def layout_cases(solver):
    S = SOLVERS[solver]
    out = [Call(solver, [5, 33, S], [[], first_sets(S, 33, 2), first_sets(S, S, 1)]).line("layout", "k3_items_0_2_1_n_5_33_s")]
    out.append(Call(solver, [], []).line("layout", "k0"))
    for n in (32, 33, 64):
        out.append(Call(solver, [n, n], [first_sets(S, n, 3), first_sets(S, n, 1)]).line("layout", f"n{n}"))
    return out


def draws_cases(S, rng):
    out = []

    def add(name, n, H, draws, mask=0):
        out.append(f"case draws{S} {name} {n} {H} {mask} {len(draws)} " + " ".join(str(int(d)) for d in draws))

    n = S + 3
    add("all_zero", n, 3, [0] * (3 * S))
    add("all_last", n, 3, [n - 1 - i for i in range(S)] * 3)
    add("same_draw_twice", n, 2, [2, 2] + [0] * (S - 2) + [1, 1] + [0] * (S - 2))
    good = [(3 * i + 1) % (n - i) for i in range(S)]
    for i in range(S):
        for what, bad in (("negative", -1), ("size", n - i)):
            add(f"refuse_{what}_at_{i}", n, 2, good + good[:i] + [bad] + good[i + 1:])
            add(f"after_refuse_{what}_at_{i}", n, 2, good + good)
    add("refuse_n_below_s", S - 1, 1, [0] * S)
    add("refuse_n_negative_without_sets", -1, 0, [])
    add("fine_n_below_s_without_sets", S - 1, 0, [])
    add("refuse_h_negative", n, -1, [])
    add("refuse_null_draws", n, 1, [0] * S, mask=1)
    add("refuse_null_sets", n, 1, [0] * S, mask=2)
    add("after_refusals", n, 1, good)
    for n in (S, S + 1, 50):
        add(f"random_n{n}", n, 200, [rng.integers(0, n - i) for _ in range(200) for i in range(S)])
    return out


def cases():
    rng = np.random.default_rng(20261021)
    out = []
    for solver in SOLVERS:
        out += check_cases(solver) + layout_cases(solver)
    for S in SOLVERS.values():
        out += draws_cases(S, rng)
    return out


def build(cxx, csrc, out):
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(csrc), "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "ransac_host_pins.cpp"), "-o", str(out)], check=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cxx", default="g++")
    ap.add_argument("--csrc", default=str(ROOT / "orb_slam2_annotate_amd" / "csrc"), help="the csrc to pin: the parent's, exported")
    args = ap.parse_args()
    lines = cases()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        build(args.cxx, Path(args.csrc), tmp / "ransac_host_pins")
        (tmp / "cases.txt").write_text("\n".join(lines) + "\n")
        subprocess.run([str(tmp / "ransac_host_pins"), str(tmp / "cases.txt"), str(tmp / "out.txt")], check=True, timeout=60)
        outs = (tmp / "out.txt").read_text().splitlines()
    assert len(outs) == len(lines)
    head = "# cases and pinned answers of tests/cpp/ransac_host_pins.cpp; see tools/gen_ransac_host_pins.py\n"
    FIXTURE.write_text(head + "".join(f"{c}\n{o}\n" for c, o in zip(lines, outs)))
    print(f"{FIXTURE}: {len(lines)} cases")


if __name__ == "__main__":
    main()
