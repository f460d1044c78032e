#!/usr/bin/env python3
"""Instruction census of the gfx950 code the product library is built from (needs hipcc, no GPU).

Compiles landing-controller_amd/csrc/capi.hip to assembly with the flags of csrc/Makefile (device side only) and prints, for every
function whose demangled name contains one of --match (default: the solver kernel and the phases of its backward sweep), what the
function is made of (and, for a function with outermost loops that hold a barrier -- the stage loops of the backward sweep -- what one
trip of each such loop is made of): instructions, instructions up to the first matrix-core instruction (operand fetch), instructions behind the last
barrier (write-out), MFMA / LDS / flat / global / branch counts, vector registers and the private segment.  For kernels the LDS block
and the private segment of the kernel descriptor are added.

    python tools/isa_census.py [--label NAME] [--match SUBSTR ...] [--asm FILE.s] [--json OUT.json]

--asm reads an assembly file made earlier instead of compiling.  --json merges the result under --label into OUT.json (so that the
census of two source states can sit side by side in one file, profiles/r08_isa_census.json).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "landing-controller_amd", "csrc")
DEFAULT_MATCH = ["block_eliminate", "last_stage_eliminate", "riccati_backward", "landing_ipm_kernel", "forward_pass"]


def makefile_flags():
    """ARCH, CXXFLAGS and HIPFLAGS as csrc/Makefile sets them"""
    var = {}
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"^(\w+)\s*[:?]?=\s*(.*)$", line.rstrip("\n"))
        if m:
            var[m.group(1)] = m.group(2).strip()
    return var.get("HIPCC", "/opt/rocm/bin/hipcc"), var.get("ARCH", "gfx950"), var["CXXFLAGS"].split(), var["HIPFLAGS"].split()


def compile_asm(out):
    hipcc, arch, cxx, hip = makefile_flags()
    hipcc = os.environ.get("HIPCC", hipcc)
    cmd = [hipcc, "--offload-arch=" + arch] + cxx + hip + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "capi.hip")]
    subprocess.run(cmd, check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    return " ".join(cmd[:-3] + ["capi.hip"]).replace(hipcc, "hipcc")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, check=True, capture_output=True, text=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


INSTR = re.compile(r"^\t([a-z][a-z0-9_]+)(\s|$)")
KD = re.compile(r"^\t\t\.amdhsa_(group_segment_fixed_size|private_segment_fixed_size|next_free_vgpr|accum_offset)\s+(\d+)")


def count_ops(ops):
    """what a list of instruction mnemonics is made of"""
    cnt = lambda f: sum(1 for o in ops if f(o))
    fp64 = {k: cnt(lambda o, k=k: o.startswith("v_" + k + "_f64")) for k in ("fma", "mul", "add", "rcp")}
    return {
        "instructions": len(ops),
        "mfma": cnt(lambda o: o.startswith("v_mfma")),
        "fp64_valu": fp64,
        "lds_read": cnt(lambda o: o.startswith("ds_read") or o.startswith("ds_load")),
        "lds_write": cnt(lambda o: o.startswith("ds_write") or o.startswith("ds_store")),
        "ds_bpermute": cnt(lambda o: o.startswith("ds_bpermute") or o.startswith("ds_permute") or o.startswith("ds_swizzle")), "dpp": cnt(lambda o: o.endswith("_dpp")),
        "flat_load": cnt(lambda o: o.startswith("flat_load")), "flat_store": cnt(lambda o: o.startswith("flat_store")),
        "global_load": cnt(lambda o: o.startswith("global_load")), "global_store": cnt(lambda o: o.startswith("global_store")),
        "scratch": cnt(lambda o: o.startswith("scratch_") or o.startswith("buffer_")),
        "branch": cnt(lambda o: o.startswith("s_cbranch") or o == "s_branch"),
        "call": cnt(lambda o: o.startswith("s_swappc")), "clock": cnt(lambda o: o.startswith("s_memrealtime") or o.startswith("s_memtime")),
        "s_waitcnt": cnt(lambda o: o == "s_waitcnt"),
        "v_cmp": cnt(lambda o: o.startswith("v_cmp")), "v_cndmask": cnt(lambda o: o.startswith("v_cndmask")),
        "exec_mask_salu": cnt(lambda o: re.match(r"s_(and|or|xor|andn2|orn2)(_saveexec)?_b64", o) is not None),
        "int_address_valu": cnt(lambda o: re.match(r"v_(add_u32|sub_u32|subrev_u32|add_co_u32|mad_u32_u24|mul_u32_u24|mad_u64_u32|lshl|lshr|ashr|or_b32|and_b32|and_or|add3|add_lshl|lshl_add|lshl_or|min_[iu]32|max_[iu]32)", o) is not None),
        "barrier": cnt(lambda o: o == "s_barrier"),
    }


LOOP_HEAD = re.compile(r"^(\.LBB\d+_\d+):\s*; =>This (?:Inner )?Loop Header: Depth=1")


BLOCK_HEAD = re.compile(r"^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)(.*)$")


def loop_blocks(body, label):
    """mnemonics of ALL blocks of the loop with header `label`, wherever the compiler laid them out: the header's block and every block
    commented `in Loop: Header=<label>` (labelled or fall-through), the loops nested in it included.  This also covers a loop whose latch block sits in FRONT of the header and
    falls through into it (the forward recursion of forward_pass), which has no branch back to the header label."""
    heads = {label[2:]}      # the loop's header and the headers of the loops nested in it (commented `Parent Loop <outer header>`)
    for line in body:
        bm = BLOCK_HEAD.match(line)
        if bm and bm.group(1) and any(("Parent Loop " + h + " ") in bm.group(2) + " " for h in list(heads)):
            heads.add(bm.group(1)[2:])
    ops, inside = [], False
    for line in body:
        bm = BLOCK_HEAD.match(line)
        if bm:
            inside = (bm.group(1) or "..")[2:] in heads or any(("Header=" + h + " ") in bm.group(2) + " " for h in heads)
        elif inside:
            mm = INSTR.match(line)
            if mm:
                ops.append(mm.group(1))
    return ops


def barrier_loops(body):
    """The outermost loops of a function that hold a barrier (the stage loops of the backward sweep, the forward recursion).  `all_blocks` =
    every block of the loop (loop_blocks).  Where the loop has a branch back to its header label it is also counted as before: `body` = from
    the loop's header label to its last back branch, `with_tail_blocks` = that plus the blocks of the loop the compiler laid out behind the
    back branch (blocks commented `in Loop: Header=<label>`; they are executed inside the loop as well)."""
    out = []
    for i, line in enumerate(body):
        m = LOOP_HEAD.match(line)
        if not m:
            continue
        label = m.group(1)
        back = max((j for j in range(i + 1, len(body)) if re.match(r"^\ts_c?branch\S*\s+" + re.escape(label) + r"\s*$", body[j].split(";")[0].rstrip())), default=None)
        if back is None:
            every = loop_blocks(body, label)
            if "s_barrier" in every:
                out.append({"header": label, "all_blocks": count_ops(every)})
            continue
        inner = [mm.group(1) for mm in (INSTR.match(b) for b in body[i:back + 1]) if mm]
        if "s_barrier" not in inner:
            continue
        tail, j, inside = [], back + 1, False
        while j < len(body):
            lm = re.match(r"^\.LBB\d+_\d+:(.*)$", body[j])
            if lm:
                inside = ("Header=" + label[2:]) in lm.group(1)
                if not inside:
                    break
            elif inside:
                mm = INSTR.match(body[j])
                if mm:
                    tail.append(mm.group(1))
            j += 1
        out.append({"header": label, "body": count_ops(inner), "with_tail_blocks": count_ops(inner + tail), "all_blocks": count_ops(loop_blocks(body, label))})
    return out


def census(path, match):
    lines = open(path, errors="replace").read().split("\n")
    funcs, kd = {}, {}
    i, n = 0, len(lines)
    while i < n:
        m = re.match(r"^\t\.type\t(\S+),@function", lines[i])
        if m:
            name = m.group(1)
            body, j = [], i + 1
            while j < n and not lines[j].startswith(".Lfunc_end"):
                mm = KD.match(lines[j])      # (a kernel's descriptor sits between its s_endpgm and the end label)
                if mm:
                    kd.setdefault(name, {})[mm.group(1)] = int(mm.group(2))
                body.append(lines[j]); j += 1
            info = {}
            while j < n and not lines[j].startswith("; MemoryBound") and not re.match(r"^\t\.type\t\S+,@function", lines[j]):
                mm = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|codeLenInByte)\s*[:=]\s*(\d+)", lines[j])
                if mm:
                    info[mm.group(1)] = int(mm.group(2))
                j += 1
            funcs[name] = (body, info)
            i = j
            continue
        i += 1
    pretty = demangle(list(funcs))
    out = {}
    for name, (body, info) in funcs.items():
        if not any(s in pretty[name] for s in match):
            continue
        ops = [m.group(1) for m in (INSTR.match(b) for b in body) if m]
        first_mfma = next((k for k, o in enumerate(ops) if o.startswith("v_mfma")), None)
        last_bar = max((k for k, o in enumerate(ops) if o == "s_barrier"), default=None)
        row = count_ops(ops)
        row.update({"to_first_mfma": first_mfma, "behind_last_barrier": None if last_bar is None else len(ops) - 1 - last_bar,
                    "vgprs": info.get("NumVgprs"), "private_segment": info.get("ScratchSize"), "code_bytes": info.get("codeLenInByte")})
        loops = barrier_loops(body)
        if loops:
            row["barrier_loops"] = loops
        if name in kd:
            row["kernel_descriptor"] = kd[name]
        out[pretty[name]] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--label", default="worktree")
    ap.add_argument("--match", nargs="*", default=DEFAULT_MATCH)
    ap.add_argument("--asm", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if a.asm:
        res, how = census(a.asm, a.match), "read from " + os.path.basename(a.asm)
    else:
        with tempfile.TemporaryDirectory() as d:
            s = os.path.join(d, "capi.s")
            how = compile_asm(s)
            res = census(s, a.match)
    keys = ["instructions", "to_first_mfma", "behind_last_barrier", "mfma", "lds_read", "lds_write", "flat_load", "flat_store", "global_load", "global_store",
            "branch", "vgprs", "private_segment"]
    print("%-58s" % "function" + "".join(" %9s" % k[:9] for k in keys))
    for f, row in sorted(res.items()):
        print("%-58s" % f[:58] + "".join(" %9s" % ("-" if row[k] is None else row[k]) for k in keys))
        for lp in row.get("barrier_loops", []):
            ab = lp["all_blocks"]
            print("    loop %s, all its blocks: %d instructions, %d barriers, LDS reads %d / writes %d, ds_bpermute %d, DPP %d, s_waitcnt %d, branches %d, global loads %d" % (
                lp["header"], ab["instructions"], ab["barrier"], ab["lds_read"], ab["lds_write"], ab["ds_bpermute"], ab["dpp"], ab["s_waitcnt"], ab["branch"], ab["global_load"]))
            if "body" not in lp:
                continue
            print("    loop %s: %d instructions to the back branch, %d with the loop's blocks behind it; clock reads %d, calls %d, scratch %d" % (
                lp["header"], lp["body"]["instructions"], lp["with_tail_blocks"]["instructions"], lp["with_tail_blocks"]["clock"], lp["with_tail_blocks"]["call"], lp["with_tail_blocks"]["scratch"]))
        if "kernel_descriptor" in row:
            print("    kernel descriptor: " + ", ".join("%s %d" % kv for kv in sorted(row["kernel_descriptor"].items())))
    if a.json:
        doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
        doc[a.label] = {"how": how, "functions": res}
        json.dump(doc, open(a.json, "w"), indent=1, sort_keys=True)
        open(a.json, "a").write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
