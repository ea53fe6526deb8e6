"""The two plan compilers, the level walk and the batched walk on the seeded corpus of tests/witness_fuzz_inputs.py, against the
independent model of tests/witness_model.py (tests/test_witness_plan_fuzz.py runs the host compiler against the same model
without a GPU).  Every comparison is exact; the expected values are the model's, never the library's.  Nothing here is meant to
fault: every input is a valid call of the public API."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import witness_fuzz_inputs as wfi  # noqa: E402
import witness_model as wm  # noqa: E402

E_ARG, E_UNSATISFIED = -7, -5
CELL = re.compile(r"\(row (\d+), column (\d+)\)")
CHUNKS = 8
BATCH_CASES = ["wide_level_d6", "mixed06", "edge_divrem_b", "seed_on_own_output"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


@pytest.fixture(scope="module")
def corpus():
    return wfi.corpus()


@pytest.fixture(scope="module")
def expected(corpus):
    return {c.name: wfi.Expected(c) for c in corpus}


def _matrix(t):
    return t.cpu().numpy().view(np.uint64)


def _want(exp):
    return np.array(exp.good[1], dtype=np.uint64)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, [(int(c), int(r), int(got[c, r]), int(want[c, r])) for c, r in bad[:6]])


def _handle(pkg, case, built):
    kw = case.circuit.kw()
    return pkg.CircuitData.build(**kw) if built else pkg.CircuitData(pkg.build_blob(**kw))


def _exported(plan, c):
    """the plan's arrays as the library exports them, and as a model Plan"""
    cell_slot, ops, level_off = plan.export()
    off, table = plan.export_generators_v()
    info = plan.info()
    counts = tuple(info[k] for k in ("ops", "levels", "widest_level", "slots", "seeds"))
    raw = [cell_slot.tobytes(), ops.tobytes(), level_off.tobytes(), off.tobytes(), table.tobytes(), counts]
    if c.gens and all(kind == "equality" for kind, _ in c.gens):
        raw.append(plan.export_generators().tobytes())            # (the record form's table: the same words)
        assert raw[-1] == table.tobytes()
    return raw, wm.Plan(cell_slot, ops, level_off, off if c.gens else None, table if c.gens else None, counts=counts)


def _both_plans(pkg, cd, case):
    """the host-compiled and the device-compiled plan: byte for byte the same arrays, valid by the model's checker"""
    c = case.circuit
    host = cd.witness_plan(case.seeds, compile="host", generators=c.generator_list())
    dev = cd.witness_plan(case.seeds, compile="device", generators=c.generator_list())
    raw_h, plan_h = _exported(host, c)
    raw_d, plan_d = _exported(dev, c)
    assert raw_h == raw_d, (case.name, [k for k, (x, y) in enumerate(zip(raw_h, raw_d)) if x != y])
    wm.check_plan(c, case.seeds, plan_h)
    wm.check_plan(c, case.seeds, plan_d)
    host.close()
    return dev, plan_d


def _failure_cell(pkg, fn):
    with pytest.raises(pkg.P2GpuError) as e:
        fn()
    assert e.value.code == E_UNSATISFIED, e.value
    row, col = CELL.findall(str(e.value))[-1]
    return int(row), int(col)


def test_the_corpus_is_the_one_the_cpu_tests_cover(corpus, expected):
    """every entry runs below: the chunks take all the solvable ones, the refusal test all the others"""
    solvable = [c for c in corpus if expected[c.name].predict == ("plan",)]
    assert len(corpus) >= 40 and len(solvable) >= CHUNKS and all(c.values is None for c in corpus if c not in solvable)
    for name in BATCH_CASES:
        assert sum(c.name.startswith(name) and c.values is not None for c in corpus) == 1, name


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_plans_and_walk(pkg, orc, gpu, corpus, expected, chunk):
    solvable = [c for c in corpus if expected[c.name].predict == ("plan",)]
    for k, case in enumerate(solvable):
        if k % CHUNKS != chunk:
            continue
        exp, c = expected[case.name], case.circuit
        cd = _handle(pkg, case, built=bool((k // CHUNKS) & 1))
        plan, model_plan = _both_plans(pkg, cd, case)
        want = _want(exp)
        got = _matrix(plan.generate(case.values))
        _same(got, want, case.name)
        # a failing value set raises and names the cell of the smallest contradiction word; the plan is as good as before afterwards
        for v in case.bad:
            cell = wm.interpret(c, case.seeds, model_plan, v)[1]
            assert cell is not None, case.name
            assert _failure_cell(pkg, lambda: plan.generate(v)) == cell, (case.name, cell)
        if case.bad:
            _same(_matrix(plan.generate(case.values)), want, case.name + " after a failure")
        # the CPU oracle's fill_witness on the routed columns (and the seeds on gate-internal ones) gives the same matrix
        routed = np.zeros_like(got)
        routed[:c.R] = got[:c.R]
        for (row, col), v in zip(case.seeds, case.values):
            if col >= c.R:
                routed[col, row] = v
        oc = orc.OracleCircuit(pkg.build_blob(**c.kw()))
        _same(np.asarray(oc.fill_witness(routed)).reshape(got.shape), got, case.name + " oracle fill")
        if case.provable:
            assert plan.prove(case.values).to_bytes() == cd.prove(got).to_bytes(), case.name
        plan.close()
        cd.close()


def test_refused_circuits(pkg, gpu, corpus, expected):
    refused = [c for c in corpus if expected[c.name].predict[0] == "refused"]
    assert len(refused) >= 8
    for k, case in enumerate(refused):
        kind, (row, col) = expected[case.name].predict[1:]
        cd = _handle(pkg, case, built=bool(k & 1))
        texts = []
        for how in ("host", "device"):
            with pytest.raises(pkg.P2GpuError) as e:
                cd.witness_plan(case.seeds, compile=how, generators=case.circuit.generator_list())
            assert e.value.code == E_ARG, e.value
            texts.append(str(e.value))
        assert texts[0] == texts[1] and kind in texts[0] and "cell (row %d, column %d)" % (row, col) in texts[0], (case.name, texts, kind, row, col)
        cd.close()


@pytest.mark.parametrize("B", [1, 3, 8, 17])
def test_batches(pkg, gpu, corpus, expected, B):
    """good and failing members in one walk: one member, a width that is no power of two, a full group, two groups and a ragged third"""
    for name in BATCH_CASES:
        (case,) = [c for c in corpus if c.name.startswith(name) and c.values is not None]
        exp, c = expected[case.name], case.circuit
        assert case.bad, name
        cd = _handle(pkg, case, built=False)
        plan = cd.witness_plan(case.seeds, compile="device", generators=c.generator_list())
        model_plan = _exported(plan, c)[1]
        fails = [(i + B) % 2 == 1 for i in range(B)]
        members = [case.bad[(i // 2) % len(case.bad)] if f else case.values for i, f in enumerate(fails)]
        got, status, bad = plan.generate_batch(members)
        want = _want(exp)
        for i, f in enumerate(fails):
            if f:
                assert status[i] == E_UNSATISFIED and bad[i] == wm.interpret(c, case.seeds, model_plan, members[i])[1], (name, i, status[i], bad[i])
            else:
                assert status[i] == 0 and bad[i] is None, (name, i)
                _same(_matrix(got[i]), want, "%s member %d" % (name, i))
        plan.close()
        cd.close()
