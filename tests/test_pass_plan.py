"""The memory plan of a Stage-B pass (gatb-core_amd/csrc/gkc_pass_plan.hpp) on its own: tests/pass_plan_driver.cpp is compiled with plain g++ against the
header and carves synthetic passes the way gkc_count_pass does. The properties checked are the ones the comments of the plan state. No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

CSRC = os.path.join(ge.ROOT, "gatb-core_amd", "csrc")
GB = 1e9


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "pass_plan_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, os.path.join(ge.ROOT, "tests", "pass_plan_driver.cpp"), "-lpthread"], check=True)
    return exe


def run(driver, parts, **kw):
    text = "".join("%s %s\n" % (k, repr(float(v)) if isinstance(v, float) else int(v)) for k, v in kw.items())
    text += "parts %d\n%s\n" % (len(parts), " ".join(str(int(v)) for v in parts))
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout
    ev = []
    for line in out.splitlines():
        w = line.split()
        if w[0] == "empty":
            ev.append(("empty", {"p": int(w[1])}))
            continue
        ev.append((w[0], {w[i]: (float(w[i + 1]) if "." in w[i + 1] else int(w[i + 1])) for i in range(1, len(w) - 1, 2)}))
    return out, ev


def uniform(n=4096, mean=2.9e6, seed=1):
    rng = np.random.default_rng(seed)
    return (mean * rng.uniform(0.8, 1.2, n)).astype(np.uint64)


def first(ev, what):
    return next(d for w, d in ev if w == what)


def batches(ev, probe=True):
    return [d for w, d in ev if w == "batch" or (probe and w == "probe")]


def check_cover(parts, ev):
    """every non-empty partition in exactly one batch, batches are runs of consecutive partitions, carved in partition order"""
    nxt = 0
    for b in batches(ev):
        assert b["consecutive"] == 1
        while nxt < len(parts) and parts[nxt] == 0:
            nxt += 1
        assert b["first"] == nxt
        inside = [p for p in range(b["first"], b["last"] + 1) if parts[p]]
        assert len(inside) == b["n"] and sum(int(parts[p]) for p in inside) == b["keys"]
        nxt = b["last"] + 1
    assert all(parts[p] == 0 for p in range(nxt, len(parts)))


def test_uniform_two_lanes(driver):
    parts = uniform()
    out, ev = run(driver, parts, avail_bytes=250 * GB)
    check_cover(parts, ev)
    st, se = first(ev, "start"), first(ev, "settled")
    assert se["lanes"] == 2
    # the memory may bind at d = 1 and no ratio is known: the probe is the first batch carved, ~0.4 % of the keys plus at most one partition
    assert st["probe_wanted"] == 1 and ev[1][0] == "probe"
    assert ev[1][1]["keys"] <= max(st["total_keys"] // 256, 16000000) and ev[1][1]["first"] == 0
    # a batch exceeds the budget only when it is a single partition
    for b in batches(ev, probe=False):
        assert b["keys"] <= se["budget"] or b["n"] == 1
    # equal inputs, equal batches (what the reuse of the allocator's blocks rests on)
    assert run(driver, parts, avail_bytes=250 * GB)[0] == out


def test_probe_in_the_queue_of_later_passes(driver):
    parts = uniform()
    _, ev = run(driver, parts, avail_bytes=250 * GB, d_hint=0.03)
    st = first(ev, "start")
    assert st["probe_pending"] == 1 and st["probe_wanted"] == 0
    b0 = batches(ev)[0]
    assert b0["first"] == 0 and b0["keys"] <= max(st["total_keys"] // 256, 16000000)
    check_cover(parts, ev)


def test_sink_ramp_and_tail(driver):
    parts = uniform()
    _, ev = run(driver, parts, avail_bytes=250 * GB, sink=1)
    check_cover(parts, ev)
    st, se = first(ev, "start"), first(ev, "settled")
    assert st["probe_pending"] == 0                      # a third of the batch size: the memory does not bind, no probe batch
    budget, lanes = se["budget"], se["lanes"]
    assert lanes == 2
    bs = batches(ev)
    for lane in range(lanes):
        mine = [b for b in bs if b["lane"] == lane]
        assert mine[0]["keys"] <= budget // 4 and mine[1]["keys"] <= budget // 2
        assert max(b["keys"] for b in mine) > budget // 2          # ... then whole ones
    for b in bs[-lanes:]:
        assert b["keys"] <= max(budget // 4, 1 << 20)
    for b in bs:
        assert b["keys"] <= budget or b["n"] == 1


def test_heavy_partitions(driver):
    parts = uniform(256, 2.0e6, seed=2)
    parts[[10, 100, 200]] = [9000000, 30000000, 12000000]
    _, ev = run(driver, parts, avail_bytes=250 * GB, batch_keys=20000000)
    check_cover(parts, ev)
    se = first(ev, "settled")
    over = [b for b in batches(ev, probe=False) if b["keys"] > se["budget"]]
    assert all(b["n"] == 1 for b in over)


def test_two_passes_plan_alike(driver):
    budgets = []
    for total in (5.2e9, 6.8e9):
        parts = uniform(4096, total / 4096, seed=3)
        _, ev = run(driver, parts, avail_bytes=250 * GB, nb_passes=2)
        check_cover(parts, ev)
        budgets.append(first(ev, "settled")["budget"])
    assert budgets[0] == budgets[1]


def test_empty_partitions(driver):
    parts = uniform(512, 3.0e5, seed=4)
    parts[::3] = 0
    parts[-5:] = 0
    _, ev = run(driver, parts, avail_bytes=250 * GB)
    check_cover(parts, ev)
    assert [d["p"] for w, d in ev if w == "empty"] == [p for p in range(len(parts)) if parts[p] == 0]        # each published once, in order


def test_forced_budget_one_lane(driver):
    parts = uniform(16, 1.0e5, seed=5)
    _, ev = run(driver, parts, avail_bytes=250 * GB, key_budget=250000, lanes=4)
    check_cover(parts, ev)
    st, se = first(ev, "start"), first(ev, "settled")
    assert st["lanes"] == 1 and se["lanes"] == 1 and st["probe_pending"] == 0 and se["slots_hint"] == 0
    for b in batches(ev):
        assert b["lane"] == 0 and (b["keys"] <= 250000 or b["n"] == 1)
    # a small input plans one lane without being told to
    _, ev = run(driver, uniform(64, 5.0e5, seed=6), avail_bytes=250 * GB, lanes=4)
    assert first(ev, "settled")["lanes"] == 1 and all(b["lane"] == 0 for b in batches(ev))


@pytest.mark.parametrize("avail_gb,d_hint,d_true", [(20, 0.0, 0.03), (60, 0.03, 0.6)])
def test_memory_binds(driver, avail_gb, d_hint, d_true):
    """little memory: one lane from the start; or (a ratio that turns out far too low) the extra lanes retire at the first batch that does not fit —
    either way lane 0 carves every partition that is left"""
    parts = uniform()
    _, ev = run(driver, parts, avail_bytes=avail_gb * GB, d_hint=d_hint, d_true=d_true)
    check_cover(parts, ev)
    se = first(ev, "settled")
    bs = batches(ev, probe=False)
    if se["lanes"] == 1:
        assert all(b["lane"] == 0 for b in bs)
    else:
        tight_from = next((i for i, b in enumerate(bs) if b["tight"]), len(bs))
        assert tight_from < len(bs), "the plan was expected to run out of room"
        assert all(b["lane"] == 0 for b in bs[tight_from + 1:])
