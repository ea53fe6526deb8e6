"""The device plan compiler's public surface, without a device: p2gpu_witness_plan_build / p2gpu_witness_plan_export in the
library and the header, their argument refusals, and WitnessPlan's `compile=` switch."""
import ctypes
import os
import re

import numpy as np
import pytest

E_ARG = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_header_signatures(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "p2gpu_witness_plan_build") and hasattr(lib, "p2gpu_witness_plan_export")
    with open(os.path.join(ROOT, "include", "p2gpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    assert ("int p2gpu_witness_plan_build(p2gpu_circuit *c, const uint32_t *seed_cells , size_t n_seeds, p2gpu_witness_plan **out);"
            in flat)
    assert ("int p2gpu_witness_plan_export(const p2gpu_witness_plan *p, uint32_t *cell_slot, uint64_t *ops, uint32_t *level_off, "
            "size_t sizes[3]);" in flat)


def test_null_arguments_need_no_device(pkg):
    lib = pkg.load_library()
    out = ctypes.c_void_p(1)
    cells = np.zeros((1, 2), dtype=np.uint32)
    assert lib.p2gpu_witness_plan_build(None, cells.ctypes.data, 1, ctypes.byref(out)) == E_ARG and not out.value
    assert lib.p2gpu_witness_plan_build(None, None, 0, None) == E_ARG
    sizes = (ctypes.c_size_t * 3)()
    assert lib.p2gpu_witness_plan_export(None, None, None, None, sizes) == E_ARG
    assert lib.p2gpu_witness_plan_export(None, None, None, None, None) == E_ARG


def test_compile_switch(pkg):
    import inspect

    assert inspect.signature(pkg.prover.WitnessPlan.__init__).parameters["compile"].default == "host"
    assert inspect.signature(pkg.prover.CircuitData.witness_plan).parameters["compile"].default == "host"
    assert callable(pkg.prover.WitnessPlan.export)
    with pytest.raises(pkg.P2GpuError) as e:
        pkg.prover.WitnessPlan(None, [], compile="gpu")          # refused before the circuit is looked at
    assert e.value.code == E_ARG and "compile" in str(e.value)


# ---- the round rule of the device level walk against the sequential rule (pure Python; DESIGN.md 6b, phase 4) ----
def _random_graph(rng):
    """ops = [(input slots, output slots, twin or None)] over a few slots; twins are neighbours, as a BaseSum row's are."""
    n_slots = int(rng.integers(2, 9))
    ops, i, n_ops = [], 0, int(rng.integers(2, 14))
    while i < n_ops:
        ins = [int(s) for s in rng.integers(0, n_slots, size=int(rng.integers(0, 3)))]
        outs = [int(s) for s in rng.integers(0, n_slots, size=int(rng.integers(0, 4)))]
        if rng.random() < 0.25 and i + 1 < n_ops:
            ops += [(ins, outs, i + 1), (outs, ins, i)]          # (each direction reads what the other sets)
            i += 2
        else:
            ops.append((ins, outs, None))
            i += 1
    return n_slots, ops


def _schedule(n_slots, ops, level_fn):
    """Both rules share everything but how one level's ready ops are decided."""
    pending = [len(ins) for ins, _, _ in ops]
    users = [[] for _ in range(n_slots)]
    for i, (ins, _, _) in enumerate(ops):
        for s in ins:
            users[s].append(i)
    slot_level, level, dead, writer = [-1] * n_slots, [-1] * len(ops), [False] * len(ops), {}
    cur, lvl = [i for i, p in enumerate(pending) if not p], 0
    while cur:
        assert lvl <= len(ops)
        nxt, fresh = level_fn(lvl, cur, ops, slot_level, level, dead, writer)
        for s in fresh:
            for u in users[s]:
                pending[u] -= 1
                if not pending[u]:
                    nxt.append(u)
        cur, lvl = sorted(nxt), lvl + 1
    return level, slot_level, writer, lvl


def _take(i, lvl, ops, slot_level, level, dead, writer, fresh):
    level[i] = lvl
    if ops[i][2] is not None:
        dead[ops[i][2]] = True
    for k, s in enumerate(ops[i][1]):
        if slot_level[s] < 0:
            slot_level[s] = lvl
            writer[s] = (i, k)
            fresh.append(s)


def _sequential_level(lvl, cur, ops, slot_level, level, dead, writer):
    nxt, fresh = [], []
    for i in cur:
        if dead[i]:
            continue
        if any(slot_level[s] == lvl for s in ops[i][1]):
            nxt.append(i)
            continue
        _take(i, lvl, ops, slot_level, level, dead, writer, fresh)
    return nxt, fresh


def _rounds_level(lvl, cur, ops, slot_level, level, dead, writer):
    nxt, fresh, undecided, rounds = [], [], list(cur), 0
    while undecided:
        rounds += 1
        assert rounds <= len(cur)
        slot_min, twin_min, contend = {}, {}, []
        for i in undecided:                                      # A (every lane sees the state the round started with)
            if dead[i]:
                continue
            if any(slot_level[s] == lvl for s in ops[i][1]):
                nxt.append(i)
                continue
            contend.append(i)
            for s in ops[i][1]:
                if slot_level[s] < 0:
                    slot_min[s] = min(slot_min.get(s, i), i)
            if ops[i][2] is not None:
                w = min(i, ops[i][2])
                twin_min[w] = min(twin_min.get(w, i), i)
        takers = [i for i in contend if all(slot_min.get(s, i) == i for s in ops[i][1])
                  and (ops[i][2] is None or twin_min[min(i, ops[i][2])] == i)]
        for i in takers:                                         # B (in any order: takers share no word)
            _take(i, lvl, ops, slot_level, level, dead, writer, fresh)
        undecided = [i for i in contend if i not in takers]
    return nxt, fresh


def test_round_rule_equals_sequential_rule():
    rng = np.random.default_rng(7)
    waited = 0
    for _ in range(400):
        n_slots, ops = _random_graph(rng)
        a = _schedule(n_slots, ops, _sequential_level)
        b = _schedule(n_slots, ops, _rounds_level)
        assert a == b, (ops, a, b)
        waited += any(l > 1 for l in a[0])
    assert waited > 100                                          # (the graphs do reach the waiting rule)
