"""What the tests share about the two libraries and about running the host emulation (test helper): where the emulation (tests/emu, the kernel sources
compiled for the host) and the product library live and how they are built, and the driver of the worker processes behind the step harnesses -- the emulation
keeps the kernels' LDS in static storage, so one process runs one launch at a time, and a harness that needs many launches starts its own file as children."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import ROOT, lc

PKG = os.path.join(ROOT, "landing-controller_amd")
CSRC = os.path.join(PKG, "csrc")
EMU_LIB = os.path.join(ROOT, "tests", "emu", "liblanding_emu.so")
PRODUCT_LIB = os.path.join(PKG, "liblanding_mi355x.so")
REF_THREADS = 16
RES = ("x", "lam_g", "iters", "status")      # the solver outputs every saved run carries, under run["res"]
_made = set()


def _run(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("command failed: %s\n%s\n%s" % (" ".join(cmd), out.stdout[-4000:], out.stderr[-4000:]))


def _make(target):
    if target not in _made:      # (make finds nothing to do the second time, but takes its time to find that out)
        _run(["make", "-C", CSRC, target])
        _made.add(target)


def build_emu():
    _make("emu")
    return EMU_LIB


def build_product():
    _make("all")
    return PRODUCT_LIB


def emu_landing_lib(N, **kw):
    return lc("capi").LandingLib(N, lib_path=build_emu(), **kw)


def is_emulation(obj):
    """obj: a LandingLib or an Rbd"""
    return hasattr(getattr(obj, "L", obj).lib, "landing_emu_set_fused")


def pool_map(fn, items, threads=REF_THREADS):
    items = list(items)
    if len(items) <= 2:
        return [fn(i) for i in items]
    with ThreadPoolExecutor(min(threads, os.cpu_count() or 1)) as ex:      # (the oracle and the sparse LU release the GIL)
        return list(ex.map(fn, items))


def compile_mex_gateway(tmp_dir, mex_source, driver_source, lib_dir, lib_name):
    """matlab/`mex_source` compiled against tests/stubs/mex.h with conftest.MexGateway's flags, together with tests/stubs/`driver_source` (None: the gateway
    alone), linked to `lib_dir`/lib`lib_name`.so; returns the shared object's path"""
    so = os.path.join(str(tmp_dir), "%s_%s.so" % (os.path.splitext(mex_source)[0], lib_name))
    stubs = os.path.join(ROOT, "tests", "stubs")
    _run(["gcc", "-O1", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-I", stubs, "-I", os.path.join(ROOT, "include"),
          os.path.join(ROOT, "matlab", mex_source)] + ([os.path.join(stubs, driver_source)] if driver_source else []) + ["-o", so, "-L", lib_dir, "-l" + lib_name, "-Wl,-rpath," + lib_dir])
    return so


# ---- worker processes: `script` is started once per job with the job as JSON in argv[1]; worker_main() is the other end
def run_workers(script, jobs, max_procs=None, label="emulation run"):
    """jobs: dicts, each with its own "out" path, in the order they are to start (the caller puts the longest first); at most min(len(jobs), CPUs, 16) children
    at a time unless max_procs says fewer.  After a child fails no further one is started, the running ones are waited for, and the first failure is raised with
    its job and the end of its output.  Returns the jobs' out paths, in the order given."""
    limit = max_procs or min(len(jobs), os.cpu_count() or 1, 16)
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    todo, running, failed = list(jobs), [], None
    while running or (todo and not failed):
        while todo and not failed and len(running) < limit:
            job = todo.pop(0)
            running.append((subprocess.Popen([sys.executable, os.path.abspath(script), json.dumps(job)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT), job))
        proc, job = running.pop(0)
        text = proc.communicate()[0]
        if proc.returncode != 0 and not failed:
            failed = (label + " failed", job, text.decode()[-2000:])
    assert not failed, failed
    return [job["out"] for job in jobs]


def worker_main(fn):
    fn(json.loads(sys.argv[1]))


def save_runs(path, runs, fields):
    """runs: {tag: run} of ONE worker, a tag being an int or a tuple of ints; of every run its res[RES] and those of `fields` it has are saved"""
    out = {"tags": json.dumps(list(runs))}
    for i, run in enumerate(runs.values()):
        out.update({"%d_%s" % (i, n): run["res"][n] for n in RES})
        out.update({"%d_%s" % (i, n): run[n] for n in fields if n in run})
    np.savez(path, **out)


def load_runs(paths, fields):
    """{tag: dict(res, **fields)} over the files of save_runs(), the parts of a tag concatenated along the member axis in the order of `paths`"""
    parts = {}
    for path in paths:
        d = np.load(path)
        for i, tag in enumerate(json.loads(str(d["tags"]))):
            parts.setdefault(tuple(tag) if isinstance(tag, list) else tag, []).append({n: d["%d_%s" % (i, n)] for n in RES + tuple(fields) if "%d_%s" % (i, n) in d})
    cat = lambda ps, names: {n: np.concatenate([p[n] for p in ps]) for n in names if n in ps[0]}
    return {tag: dict(cat(ps, fields), res=cat(ps, RES)) for tag, ps in parts.items()}
