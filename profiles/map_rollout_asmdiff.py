#!/usr/bin/env python3
"""Are the kernels of two builds the same code?  Compares, kernel by kernel, the device assembly of two `hipcc -S
--cuda-device-only` outputs of csrc/cagpu.hip (same flags as build_native.FLAGS without -shared) -- the whole text of every
kernel body, nothing instruction-specific:

    hipcc <FLAGS> --cuda-device-only -S gym_collision_avoidance_amd/csrc/cagpu.hip -o new.s      (and the same in the parent tree)
    python profiles/map_rollout_asmdiff.py parent.s new.s [-v]

Comments are dropped; labels that carry a file-wide ordinal (.LBB<function>_<n>, .Lpost_getpc<n>, jump tables) are
renamed, since adding a function shifts them, and so is a kernel's own mangled symbol inside its body; a kernel is
matched by its demangled name, and the trailing template argument MSET = false of ca_kernel and ca_pipe_kernel counts
as the parent's instantiation without it.  Prints the kernels that differ, exist on
one side only, and -- with -v -- the identical ones, each with (next_free_vgpr, accum_offset, scratch bytes per lane =
private_segment_fixed_size) of both builds."""
import re
import subprocess
import sys


def bodies(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and cur is None:
            name, cur = m.group(1), []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                out[name], cur = cur, None
            else:
                cur.append(line)
    return out


def norm(lines):
    res = []
    for l in lines:
        l = l.split(";")[0].rstrip()
        if l.strip():
            l = re.sub(r"\.(LBB|LJTI|LCPI)\d+_", r".\1_", l)
            l = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", l)
            res.append(re.sub(r"_ZN\w*ca_(pipe_)?kernel\w*", "SELF", l))   # (a body names its own symbol, which spells every template argument)
    return res


def vgprs(path):
    d = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(path).read(), re.S):
        v = re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2))
        a = re.search(r"\.amdhsa_accum_offset (\d+)", m.group(2))
        p = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
        d[m.group(1)] = (int(v.group(1)), int(a.group(1)) if a else None, int(p.group(1)) if p else 0)
    return d


def load(path):
    b, v = bodies(path), vgprs(path)
    names = sorted(v)
    dem = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()))

    def key(n):
        d = dem[n].replace("(anonymous namespace)::", "").replace("(KArgs)", "")
        if ("ca_kernel<" in d or "ca_pipe_kernel<" in d) and d.count(",") == 6:
            d = re.sub(r", false>", ">", d)
        return d
    return {key(n): norm(b[n]) for n in names}, {key(n): v[n] for n in names}


def main():
    (P, vp), (N, vn) = load(sys.argv[1]), load(sys.argv[2])
    same = diff = 0
    for n in sorted(set(P) | set(N)):
        if n not in P:
            print("NEW  ", n, "vgpr", vn[n])
        elif n not in N:
            print("GONE ", n)
        elif P[n] == N[n]:
            same += 1
            if "-v" in sys.argv:
                print("SAME ", n, len(P[n]), "lines, vgpr", vp[n], vn[n])
        else:
            diff += 1
            print("DIFF ", n, len(P[n]), "->", len(N[n]), "lines, vgpr", vp[n], "->", vn[n])
    print("identical: %d, different: %d, new: %d, gone: %d" % (same, diff, len(set(N) - set(P)), len(set(P) - set(N))))


if __name__ == "__main__":
    main()
