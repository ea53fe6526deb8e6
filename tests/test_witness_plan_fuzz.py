"""The witness plan on a seeded corpus of random circuits, without a GPU: the stand-alone printer of the host compiler
(csrc/tests/planhost_print.cpp, g++ only; the plain build and one with -fsanitize=address,undefined, as
test_witness_plan_generators.py builds them) against the independent model of tests/witness_model.py.
  a circuit the model expects to compile: its plan passes `check_plan`, and the plan run by `interpret` gives the matrix of the
  plan-free `evaluate` on the good value set and names a contradiction exactly on the failing ones;
  a circuit the model expects to be refused: the printer refuses it with that kind and that cell;
  the recorded plans pass the checker, six corruptions of a plan do not, a subtly wrong generator body is noticed;
  the corpus covers what it is meant to cover -- counted by the model alone, never by the code under test.
Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import device_build_inputs as dbi  # noqa: E402
import gate_wires as gw  # noqa: E402
import witness_fuzz_inputs as wfi  # noqa: E402
import witness_gen_inputs as wgi  # noqa: E402
import witness_model as wm  # noqa: E402
import witness_plan_inputs as wpi  # noqa: E402
import witness_plan_recorded as wpr  # noqa: E402
from test_witness_plan_divrem import run_v  # noqa: E402
from test_witness_plan_generators import printer, run_printer  # noqa: E402,F401  (the fixture builds both printers)

W = wm.WRITER


@pytest.fixture(scope="module")
def corpus():
    cases = wfi.corpus()
    assert [c.name for c in cases] == [c.name for c in wfi.corpus()]           # deterministic
    return cases


@pytest.fixture(scope="module")
def expected(corpus):
    return {c.name: wfi.Expected(c) for c in corpus}


def compile_case(exe, tmp_path, pkg, case):
    """the printer on the case: ("plan", wm.Plan) or ("refused", text)"""
    c = case.circuit
    blob = pkg.build_blob(**c.kw())
    if c.gens:
        recs = np.array([[wm.GEN_KIND[kind], *c.gen_shape(g)] for g, (kind, _) in enumerate(c.gens)], dtype=np.uint32)
        flat = np.array([cell for g in range(len(c.gens)) for cell in c.gen_cells(g)], dtype=np.uint32)
        got = run_v(exe, tmp_path, blob, case.seeds, recs, flat)
    else:
        got = run_printer(exe, tmp_path, blob, case.seeds)
    if got[0] == "refused":
        return got
    arrays = got[2]
    return "plan", wm.Plan(arrays[0], arrays[1], arrays[2], *(arrays[3:5] if c.gens else (None, None)), counts=got[1])


# ---- the model itself -----------------------------------------------------------------------------------------------------------------
def test_bodies_agree_with_gate_wires():
    """the five custom-gate bodies on the inputs tests/gate_wires.py defines (the reference's own `get_wires` helpers)"""
    F = 0xFFFFFFFF

    def row(kind, p, inputs):
        """the gate's ops on a row whose input columns hold `inputs`"""
        w = dict(inputs)
        for code, sub, ins, outs in wm.row_ops(kind, p):
            sets, rej = wm.BODY[code](p, sub, lambda col: w.get(col, 0), None)
            assert not rej
            w.update(sets)
        return [w.get(col, 0) for col in range(wm.gate_wires_used(kind, p))]

    m0, m1, ad = [0, 1, F, 0x12345678], [0, F, F, 0x9ABCDEF0], [0, 1, F, 77]
    want = gw.u32_arithmetic_wires(m0, m1, ad)
    assert row(wm.G_U32_ARITHMETIC, (4,), {6 * i + k: v[i] for i in range(4) for k, v in enumerate((m0, m1, ad))}) == want
    addends, carries = [[F, F, 5], [1, 2, 3], [0, 0, 0]], [3, 0, 1]
    want, na = gw.u32_add_many_wires(addends, carries)
    assert row(wm.G_U32_ADD_MANY, (na, 3), {(na + 3) * i + j: v for i in range(3) for j, v in enumerate(addends[i] + [carries[i]])}) == want
    xs, ys, bs = [5, 0, F, 1 << 31], [7, 0, F, 1], [0, 1, 1, 0]
    assert row(wm.G_U32_SUBTRACTION, (4,), {5 * i + k: v[i] for i in range(4) for k, v in enumerate((xs, ys, bs))}) == gw.u32_subtraction_wires(xs, ys, bs)
    limbs = [0, 1, F, 0xDEADBEEF]
    assert row(wm.G_U32_RANGE_CHECK, (4,), dict(enumerate(limbs))) == gw.u32_range_check_wires(limbs)
    for a, b, nb, nc in ((5, 9, 4, 2), (9, 5, 4, 2), (7, 7, 3, 3), (0x80000000, 0x7FFFFFFF, 32, 16), (1234567, 1234568, 21, 7), (3, 0, 7, 2)):
        assert row(wm.G_COMPARISON, (nb, nc), {0: a, 1: b}) == [v % wm.P for v in gw.comparison_wires(a, b, nb, nc)], (a, b, nb, nc)


def test_poseidon_body_gives_the_committed_permutations():
    import json

    with open(os.path.join(HERE, "golden", "poseidon.json")) as f:
        vectors = json.load(f)["permutation_vectors"]
    for v in vectors:
        assert wm.poseidon_permute(v["input"]) == v["output"]
    # swap = 1 exchanges the two halves of the rate before the permutation
    st = [wm.P - 1] * 4 + [1, 2, 3, 4] + [0] * 4
    out = dict(wm.body_poseidon((), 0, lambda col: (st + [0] * 12 + [1])[col], None)[0])
    assert [out[12 + i] for i in range(12)] == wm.poseidon_permute(st[4:8] + st[:4] + st[8:])


def test_registry_matches_the_bodies():
    """every column a body sets is an output column of its op and every output column is set; what it reads is an input column"""
    rng = __import__("random").Random(5)
    b = wfi.Builder(rng, 2)
    for kind in wfi.KINDS:
        for _ in range(6):
            p = b.params(kind)
            for code, sub, ins, outs in wm.row_ops(kind, p):
                read = []
                sets, _ = wm.BODY[code](p, sub, lambda col: read.append(col) or 1, lambda i: 1)
                assert sorted(col for col, _ in sets) == sorted(outs) and len(sets) == len(outs), (kind, p, code)
                assert set(read) <= set(ins), (kind, p, code)


# ---- coverage: the model alone ------------------------------------------------------------------------------------------------------
def test_corpus_covers_what_it_is_meant_to(corpus, expected):
    solvable = [c for c in corpus if expected[c.name].predict == ("plan",)]
    refused = [c for c in corpus if expected[c.name].predict[0] == "refused"]
    assert len(corpus) >= 40 and len(solvable) >= 0.8 * len(corpus)
    assert all(c.values is None for c in refused) and all(c.values is not None for c in solvable)
    for kind in ("a seed is missing", "dependency cycle"):
        assert sum(expected[c.name].predict[1] == kind for c in refused) >= 4, kind
    assert all(expected[c.name].good[0] == "ok" for c in solvable)
    # every op code is scheduled in at least 3 plans
    for code in range(15):
        assert sum(any(ops[0] == code for k, ops in enumerate(expected[c.name].schedule["ops"]) if k in expected[c.name].schedule["level"])
                   for c in solvable) >= 3, code
    # every gate kind that has parameters appears with at least 3 parameter sets (PoseidonGate has none: its rows count instead)
    for kind in wfi.KINDS:
        params = {p for c in solvable for k, p, _, _ in c.circuit.gates if k == kind}
        rows = sum(c.circuit.gate(r)[0] == kind for c in solvable for r in range(c.circuit.n))
        assert (len(params) >= 3) if kind != wm.G_POSEIDON else rows >= 3, (kind, params)
    base, chunk, addends, ra = (({p for c in solvable for k, p, _, _ in c.circuit.gates if k == kind}) for kind in
                                (wm.G_BASE_SUM, wm.G_COMPARISON, wm.G_U32_ADD_MANY, wm.G_RANDOM_ACCESS))
    assert {b for b, _ in base} == set(range(2, 9)) and {1, 64} <= {lm for _, lm in base}
    assert {-(-nb // nc) for nb, nc in chunk} == {1, 2, 3, 4} and any(nb % nc for nb, nc in chunk)
    assert {0, 16} <= {na for na, _ in addends}
    assert {bits for bits, _, _ in ra} == set(range(1, 7)) and {e for _, _, e in ra} == {0, 1, 2}
    assert {c.circuit.d for c in solvable} == {2, 3, 4, 5, 6} and {(234, 80), (135, 80)} <= {(c.circuit.W, c.circuit.R) for c in solvable}
    assert any(c.circuit.R != 80 for c in solvable)
    arith = [(c.circuit.lc(r, 0), c.circuit.lc(r, 1)) for c in solvable for r in range(c.circuit.n) if c.circuit.gate(r)[0] == wm.G_ARITHMETIC]
    assert sum(c0 == 0 for c0, _ in arith) >= 3 and sum(c1 == 0 for _, c1 in arith) >= 3
    # the deliberate structure, in at least 3 circuits each (the wide level: in 1)
    count = dict.fromkeys(("two_derive", "op_waits", "limbs_first", "generator_shares_output", "seed_on_derived", "slotless_input", "seed_high_column",
                           "wide_level", "poseidon_swap0", "poseidon_swap1", "equality", "divrem"), 0)
    for c in solvable:
        sch, cc = expected[c.name].schedule, c.circuit
        S, ops, level = sch["S"], sch["ops"], sch["level"]
        by_root = {}
        for k in level:
            for cell in ops[k][4]:
                by_root.setdefault(S.root(cell), set()).add(k)
        row_outs = {cell for k in level for cell in ops[k][4] if ops[k][0] not in (wm.OP_SEED, wm.OP_EQUALITY, wm.OP_BIGUINT_DIVREM)}
        derived = {r for r, ks in by_root.items() if any(ops[k][0] != wm.OP_SEED for k in ks)}
        swaps = {expected[c.name].good[1][24][r] for r in range(cc.n) if cc.gate(r)[0] == wm.G_POSEIDON}
        found = dict(two_derive=any(sum(ops[k][0] != wm.OP_SEED for k in ks) >= 2 for ks in by_root.values()),
                     op_waits=bool(sch["waited"]), limbs_first=bool(sch["joins"]),
                     generator_shares_output=any(cell in row_outs for g in range(len(cc.gens)) for cell in cc.gen_cells(g)[-sum(cc.gen_shape(g)[2:]):]),
                     seed_on_derived=any(s[1] < cc.R and S.root(s) in derived for s in c.seeds),
                     slotless_input=any(col < cc.R and cc.key((r, col)) not in S.slotted for k in level if ops[k][0] not in (wm.OP_SEED, wm.OP_EQUALITY, wm.OP_BIGUINT_DIVREM)
                                        for r in [ops[k][1]] for code, sub, ins, _ in wm.row_ops(*cc.gate(r)[:2], cc.lc(r, 0), cc.lc(r, 1))
                                        if (code, sub) == (ops[k][0], ops[k][2]) for col in ins),
                     seed_high_column=any(s[1] >= cc.R for s in c.seeds), wide_level=sch["widest"] > 512,
                     poseidon_swap0=0 in swaps, poseidon_swap1=1 in swaps,
                     equality=any(k == "equality" for k, _ in cc.gens), divrem=any(k == "biguint_divrem" for k, _ in cc.gens))
        for key, hit in found.items():
            count[key] += bool(hit)
    assert all(v >= (1 if key == "wide_level" else 3) for key, v in count.items()), count
    assert {cc.gen_shape(g) for c in solvable for cc in [c.circuit] for g in range(len(cc.gens))} >= {(1, 1, 1, 1), (3, 2, 2, 2), (2, 4, 0, 4)}
    # every edge word reaches an input of every kind of generator that has inputs
    seen = {}
    for c in solvable:
        for code, read in expected[c.name].trace:
            seen.setdefault(code, set()).update(read)
    for code in range(1, 15):
        if code not in (wm.OP_CONSTANT, wm.OP_RA_CONSTS):
            assert set(wfi.EDGE_WORDS) <= seen.get(code, set()), (code, sorted(set(wfi.EDGE_WORDS) - seen.get(code, set())))
    # failing value sets: on a third of the solvable circuits at least, all three sorts; every one is a contradiction to the model
    assert sum(bool(c.bad) for c in solvable) * 3 >= len(solvable)
    sorts = [r for c in solvable for r in expected[c.name].bad]
    assert all(r[0] == "contradiction" for r in sorts) and {r[1] for r in sorts} == {"compare", "reject", "noncanonical"}


# ---- the host compiler against the model --------------------------------------------------------------------------------------------
def test_every_circuit_compiles_or_is_refused_as_the_model_says(pkg, printer, corpus, expected, tmp_path):  # noqa: F811
    wrong = []
    for case in corpus:
        exp, c = expected[case.name], case.circuit
        got = compile_case(printer, tmp_path, pkg, case)
        if exp.predict[0] == "refused":
            kind, (row, col) = exp.predict[1:]
            if not (got[0] == "refused" and kind in got[1] and "cell (row %d, column %d)" % (row, col) in got[1]):
                wrong.append((case.name, "refusal", exp.predict, got[:2]))
            continue
        if got[0] != "plan":
            wrong.append((case.name, "refused", got[1]))
            continue
        try:
            wm.check_plan(c, case.seeds, got[1])
        except wm.PlanError as e:
            wrong.append((case.name, "check_plan", str(e)))
            continue
        m, cell = wm.interpret(c, case.seeds, got[1], case.values)
        if cell is not None or m != exp.good[1]:
            wrong.append((case.name, "good set", cell, [(col, row) for col in range(c.W) for row in range(c.n) if m[col][row] != exp.good[1][col][row]][:4]))
        for k, v in enumerate(case.bad):
            if wm.interpret(c, case.seeds, got[1], v)[1] is None:
                wrong.append((case.name, "failing set %d goes unnoticed" % k, exp.bad[k]))
    assert not wrong, wrong


def test_recorded_plans_pass_the_checker(pkg):
    recorded, cases = wpr.load(os.path.join(HERE, "golden")), wpr.cases(pkg)
    checked = 0
    for name, (blob, cells) in cases.items():
        if name in wpr.DIGEST_ONLY:
            continue
        kw = wpi.HAND_BUILT[name]()[0] if name in wpi.HAND_BUILT else wgi.custom_gate_chain()[0] if name == "custom_gate_chain" else dbi.decompose(pkg, blob)
        c, rec = wm.Circuit.from_kw(kw), recorded[name]
        assert wm.predict(c, cells) == ("plan",), name
        wm.check_plan(c, cells, wm.Plan(rec["cell_slot"].reshape(c.R, c.n), rec["ops"], rec["level_off"], counts=rec["counts"]))
        checked += 1
    assert checked == len(cases) - len(wpr.DIGEST_ONLY) >= 10


# ---- the checker and the oracle have teeth --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans(pkg, corpus, tmp_path_factory):
    """the plans of a few corpus circuits through a plain build of the printer"""
    import subprocess

    exe = str(tmp_path_factory.mktemp("planhost_teeth") / "planhost_print")
    src = os.path.join(os.path.dirname(HERE), "acvm-backend-plonky2_amd", "csrc", "tests", "planhost_print.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src], check=True, timeout=600)
    tmp = tmp_path_factory.mktemp("teeth")
    out = {}
    for case in corpus:
        if case.values is not None and case.name.startswith(("mixed", "edge_equality", "borrow_boundary", "seed_on_own_output")):
            got = compile_case(exe, tmp, pkg, case)
            assert got[0] == "plan", got
            info = wm.check_plan(case.circuit, case.seeds, got[1])
            out[case.name] = (case, got[1])
            # the corruptions below need a BaseSum row, an op that compares and a third level
            codes = {code for _, code, _ in got[1].decoded()}
            compares = any(info["writer"][info["want"][case.circuit.key(cell)]][1] != k for k in info["level"] for cell in info["ops"][k][4])
            if case.name.startswith("mixed") and codes & {wm.OP_BASE_SPLIT, wm.OP_BASE_JOIN} and compares and info["levels"] >= 4:
                out["corrupt%d" % sum(k.startswith("corrupt") for k in out)] = (case, got[1])
    return out


def _rejected(case, plan):
    with pytest.raises(wm.PlanError):
        wm.check_plan(case.circuit, case.seeds, plan)


@pytest.mark.parametrize("name", ["corrupt0", "corrupt1", "corrupt2"])
def test_check_plan_rejects_corrupted_plans(plans, name):
    case, plan = plans[name]
    c = case.circuit
    info = wm.check_plan(c, case.seeds, plan)
    ops, level, writer, want = info["ops"], info["level"], info["writer"], info["want"]
    row_writers = [(s, w) for s, w in sorted(writer.items()) if ops[w[1]][0] not in (wm.OP_EQUALITY, wm.OP_BIGUINT_DIVREM)]
    # 1. a writer bit cleared
    s, (lvl, k, pos) = row_writers[len(row_writers) // 2]
    row, col = ops[k][4][pos]
    q = plan.copy()
    q.cell_slot[col][row] &= ~W
    _rejected(case, q)
    # 2. a second writer bit: on a cell of an op that compares
    compares = [(k, pos) for k in level for pos, cell in enumerate(ops[k][4]) if ops[k][0] not in (wm.OP_SEED, wm.OP_EQUALITY, wm.OP_BIGUINT_DIVREM)
                and writer[want[c.key(cell)]][1:] != (k, pos) and cell not in case.seeds]
    assert compares, "the corpus circuit holds no comparing op"
    k, pos = compares[0]
    row, col = ops[k][4][pos]
    q = plan.copy()
    q.cell_slot[col][row] |= W
    _rejected(case, q)
    # 3. an op moved one level down, into the level of its input's writer
    lo = plan.level_off
    moved = next(lvl for lvl in range(2, len(lo) - 1) if lo[lvl + 1] - lo[lvl] >= 1 and lo[lvl] - lo[lvl - 1] >= 1)
    q = plan.copy()
    q.level_off[moved] += 1                      # (the first op of level `moved` now closes the level below)
    _rejected(case, q)
    # 4. two ops of one level out of creation order
    lvl = next(lvl for lvl in range(len(lo) - 1) if lo[lvl + 1] - lo[lvl] >= 2)
    q = plan.copy()
    q.ops[lo[lvl]], q.ops[lo[lvl] + 1] = q.ops[lo[lvl] + 1], q.ops[lo[lvl]]
    _rejected(case, q)
    # 5. two classes in one slot
    q = plan.copy()
    cells = [(col, row) for col in range(c.R) for row in range(c.n) if plan.cell_slot[col][row] != wm.UNSET]
    (c0, r0), (c1, r1) = cells[0], next(x for x in cells if plan.cell_slot[x[0]][x[1]] & ~W != plan.cell_slot[cells[0][0]][cells[0][1]] & ~W)
    q.cell_slot[c1][r1] = (q.cell_slot[c1][r1] & W) | (q.cell_slot[c0][r0] & ~W)
    _rejected(case, q)
    # 6. a BaseSum row's direction flipped
    flip = [pos for pos, (idx, code, sub) in enumerate(plan.decoded()) if code in (wm.OP_BASE_SPLIT, wm.OP_BASE_JOIN)]
    assert flip, "the corpus circuit holds no BaseSum row"
    q = plan.copy()
    idx, code, sub = plan.decoded()[flip[0]]
    q.ops[flip[0]] = idx | ((wm.OP_BASE_SPLIT + wm.OP_BASE_JOIN - code) << 32)
    _rejected(case, q)
    # and further: an op dropped, a count that the arrays do not have, a generator's table word on another cell
    q = plan.copy()
    del q.ops[-1]
    q.level_off[-1] -= 1
    _rejected(case, q)
    q = plan.copy()
    q.counts = q.counts[:3] + (q.counts[3] + 1,) + q.counts[4:]
    _rejected(case, q)


def test_check_plan_rejects_a_corrupted_generator_table(plans):
    case, plan = plans["edge_equality"]
    q = plan.copy()
    q.gen_table[2] &= ~W                          # the first generator's `equal`: nobody writes it now
    _rejected(case, q)
    q = plan.copy()
    q.gen_table[0] |= W                           # a writer bit on an input
    _rejected(case, q)
    q = plan.copy()
    q.gen_table[3] = (q.gen_table[3] & W) | (q.gen_table[7] & ~W)
    _rejected(case, q)


def test_a_subtly_wrong_body_is_noticed(plans, monkeypatch):
    """`>=` in place of `>` in the subtraction's borrow: the plan's interpreter and the plan-free evaluation part ways"""
    case, plan = plans["borrow_boundary"]
    good = wm.evaluate(case.circuit, case.seeds, case.values)
    assert good[0] == "ok" and wm.interpret(case.circuit, case.seeds, plan, case.values) == (good[1], None)

    def wrong(p, i, get, lc):
        init = (get(5 * i) - get(5 * i + 1) - get(5 * i + 2)) % wm.P
        borrow = 1 if init >= 1 << 32 else 0
        res = (init + (borrow << 32)) % wm.P
        return [(5 * i + 3, res), (5 * i + 4, borrow)] + [(5 * p[0] + 16 * i + j, (res >> (2 * j)) & 3) for j in range(16)], []
    monkeypatch.setitem(wm.BODY, wm.OP_U32_SUBTRACTION, wrong)
    m, cell = wm.interpret(case.circuit, case.seeds, plan, case.values)
    assert cell is None and m != good[1]
    bad = {(row, col) for col in range(case.circuit.W) for row in range(case.circuit.n) if m[col][row] != good[1][col][row]}
    assert bad and {col // 5 for row, col in bad if col < 20} == {0, 1}          # the two operations whose difference is exactly 2^32


def test_a_seed_on_an_op_s_own_output_is_compared(plans):
    """the named case: the wrong seed value on the operation's output cell names that cell"""
    case, plan = plans["seed_on_own_output"]
    for v in case.bad:
        assert wm.evaluate(case.circuit, case.seeds, v) == ("contradiction", "compare")
        (k,) = [k for k in range(len(v)) if v[k] != case.values[k]]
        assert wm.interpret(case.circuit, case.seeds, plan, v)[1] == case.seeds[k]
