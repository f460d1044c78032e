"""CPU tests of tests/emu_support.py itself: the worker-process driver with a throw-away worker script (no emulation involved), the memoised build and the
save_runs / load_runs pair."""
import os
import subprocess

import numpy as np
import pytest

import emu_support as E

# the worker: writes its tag through save_runs; "after": first waits (bounded) until that file exists, so that it finishes AFTER a job started behind it;
# "fail": prints a line and exits 3 instead
WORKER = """
import os, sys, time
sys.path.insert(0, %r)
import numpy as np
import emu_support as E

def work(job):
    t0 = time.time()
    while job.get("after") and not os.path.exists(job["after"]):
        assert time.time() - t0 < 20
        time.sleep(0.005)
    if job.get("fail"):
        print("the worker's last words, tag %%d" %% job["tag"])
        sys.exit(3)
    z = np.full((1, 2), float(job.get("val", 0)))
    E.save_runs(job["out"], {job["tag"]: dict(res={n: z for n in E.RES})}, ())

E.worker_main(work)
""" % os.path.dirname(os.path.abspath(__file__))


@pytest.fixture()
def script(tmp_path):
    p = tmp_path / "worker.py"
    p.write_text(WORKER)
    return str(p)


def test_results_come_back_in_the_order_of_the_jobs(script, tmp_path):
    out = [str(tmp_path / ("%d.npz" % i)) for i in range(3)]
    jobs = [dict(tag=7, val=0, out=out[0], after=out[2]), dict(tag=7, val=1, out=out[1], after=out[2]), dict(tag=7, val=2, out=out[2])]      # the last one finishes first
    paths = E.run_workers(script, jobs, max_procs=3)
    assert paths == out
    runs = E.load_runs(paths, ())
    assert list(runs) == [7] and np.array_equal(runs[7]["res"]["x"], [[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]])      # the members of a tag, in the order of the jobs


def test_a_failing_child_is_reported_and_nothing_behind_it_starts(script, tmp_path):
    out = [str(tmp_path / ("%d.npz" % i)) for i in range(3)]
    jobs = [dict(tag=0, out=out[0]), dict(tag=1, out=out[1], fail=True), dict(tag=2, out=out[2])]
    with pytest.raises(AssertionError) as e:
        E.run_workers(script, jobs, max_procs=1, label="throw-away run")
    text = str(e.value)
    assert "throw-away run failed" in text and out[1] in text and "the worker's last words, tag 1" in text
    assert os.path.exists(out[0]) and not os.path.exists(out[1]) and not os.path.exists(out[2])


def test_build_emu_runs_make_once(monkeypatch):
    calls = []

    def fake_run(cmd, **kw):
        calls.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, "", "")
    monkeypatch.setattr(E, "_made", set())
    monkeypatch.setattr(subprocess, "run", fake_run)
    assert E.build_emu() == E.EMU_LIB and E.build_emu() == E.EMU_LIB
    assert calls == [["make", "-C", E.CSRC, "emu"]]
    assert E.build_product() == E.PRODUCT_LIB and len(calls) == 2 and calls[1][-1] == "all"


def test_a_failing_build_shows_the_compiler_output(monkeypatch):
    monkeypatch.setattr(E, "_made", set())
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: subprocess.CompletedProcess(cmd, 2, "make: out", "kernel.hip:3: error: expected ';'"))
    with pytest.raises(RuntimeError, match="command failed: make -C .* emu\n(.|\n)*expected ';'"):
        E.build_emu()
    assert not E._made      # a failed build is not remembered


def test_save_and_load_runs_round_trip(tmp_path):
    """two members (files), two tags -- an int and a tuple --, and an optional field whose length differs between the members and which only one tag carries"""
    rng = np.random.default_rng(0)
    res = lambda: {n: rng.normal(size=(1, 3)) for n in E.RES}
    members = [{5: dict(res=res(), ws=rng.normal(size=(1, 4)), Jb=rng.normal(size=(k, 2))), (2, 3): dict(res=res(), ws=rng.normal(size=(1, 4)), off="not a field")} for k in (1, 3)]
    paths = [str(tmp_path / ("m%d.npz" % i)) for i in range(2)]
    for p, m in zip(paths, members):
        E.save_runs(p, m, ("ws", "Jb"))
    runs = E.load_runs(paths, ("ws", "Jb"))
    assert list(runs) == [5, (2, 3)]
    for tag in runs:
        for n in E.RES:
            assert np.array_equal(runs[tag]["res"][n], np.concatenate([m[tag]["res"][n] for m in members]))
        assert np.array_equal(runs[tag]["ws"], np.concatenate([m[tag]["ws"] for m in members]))
    assert runs[5]["Jb"].shape == (4, 2) and np.array_equal(runs[5]["Jb"], np.concatenate([m[5]["Jb"] for m in members]))
    assert sorted(runs[2, 3]) == ["res", "ws"]
    back = E.load_runs(paths[::-1], ("ws",))      # the order of the paths is the order of the members
    assert np.array_equal(back[5]["ws"], np.concatenate([m[5]["ws"] for m in members[::-1]])) and "Jb" not in back[5]
