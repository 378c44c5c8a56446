#!/usr/bin/env python3
r"""Compare the kernels of two gfx950 assembly listings function by function.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -S --cuda-device-only \
          -o engine.s mops_amd/csrc/mops_engine.hip      (and -o analysis.s mops_amd/csrc/mops_analysis.hip)
    cat engine.s analysis.s > new.s                      (the same for the parent's sources: parent.s)
    python tools/asm_compare.py parent.s new.s [--rename REGEX REPLACEMENT]

Every function of the first listing must exist in the second with the same body once comments, debug
directives and the numbering of local labels (.LBB<n>_, .Lfunc_begin<n>, .Ltmp<n>, .Lpost_getpc<n>) are
normalised.  Functions only the second listing has (new kernels) are listed, not compared.  Exit status 1 when a
function of the first listing is missing or differs: the PMC records in profiles/pmc_traffic.json belong to the
device code, so they may be re-stamped to a new build id (same_device_code_as) only when this passes.

--rename: re.sub(REGEX, REPLACEMENT) on the second listing's function names, and on the lines of their bodies (a
kernel's descriptor and section directives repeat its name), before the comparison: for a change that only
re-mangles names.  traj_kernel's trailing template parameter CAP = false and its parameter type
std::conditional_t<CAP, TrajArgsCap, TrajArgs> do that to every instantiation:
    --rename '_Z11traj_kernelI(Li\d+E)((?:Lb[01]E){4})Lb0EEv\w+' '_Z11traj_kernelI\1\2Ev8TrajArgs'
A renamed name that collides with another function of the second listing is an error.
"""
import hashlib
import re
import sys


def functions(path):
    out, cur, body, typed = {}, None, [], None
    for line in open(path):
        t = re.match(r"^\s*\.type\s+(\w+),@function", line)
        if t:
            typed = t.group(1)
        m = re.match(r"^([A-Za-z_]\w*):\s*(;.*)?$", line)
        if m and cur is None and m.group(1) == typed:  # (not a data label: another listing's functions may follow it)
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[cur] = body
                cur = None
                continue
            s = re.sub(r";.*$", "", line).rstrip()
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)
            s = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", s)
            s = re.sub(r"\.Ltmp\d+", ".Ltmp", s)
            s = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", s)
            if s.strip() and not s.strip().startswith((".loc", ".file", ".cfi")):
                body.append(s)
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    if len(sys.argv) > 3:
        if len(sys.argv) != 6 or sys.argv[3] != "--rename":
            sys.exit(__doc__)
        renamed = {}
        for name, body in b.items():
            new = re.sub(sys.argv[4], sys.argv[5], name)
            if new in renamed or (new != name and new in b):
                sys.exit(f"--rename: {name} -> {new} collides")
            renamed[new] = [re.sub(sys.argv[4], sys.argv[5], ln) for ln in body]
            if new != name:
                print("renamed in the second listing:", name, "->", new)
        b = renamed
    bad = 0
    h = hashlib.sha256()
    for name in sorted(a):
        h.update(name.encode())
        h.update("\n".join(a[name]).encode())
        if name not in b:
            print("MISSING in the second listing:", name)
            bad += 1
        elif a[name] != b[name]:
            print("DIFFERENT:", name, len(a[name]), "->", len(b[name]), "lines")
            bad += 1
    print(f"functions in the first listing: {len(a)}; identical in the second: {len(a) - bad}; "
          f"missing or different: {bad}")
    print("normalised lines compared:", sum(len(v) for v in a.values()))
    print("sha256 of the first listing's normalised functions:", h.hexdigest())
    for name in sorted(set(b) - set(a)):
        print("only in the second listing:", name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
