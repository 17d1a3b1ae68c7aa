"""VALU census of the 1-D programme loops (p2b_round, csrc/cagpu_pipe.inc) in a device assembly listing.

    hipcc <FLAGS of build_native.py without -shared / -fPIC> -S --cuda-device-only csrc/cagpu.hip -o cagpu.s
    python profiles/p2b_loop_census.py cagpu.s [--kernel MANGLED_SUBSTRING] [--list]

A loop is taken from the compiler's own block comments: its header block ("This Inner Loop Header") and every block marked
"in Loop: Header=<that header>".  The loops of p2b_round are the innermost loops of the kernel that hold LDS reads and
v_rcp_f32 in PAIRS and nothing else transcendental (the two divide chains of a pair of lines); one trip of such a loop may hold
several pairs (the loop is unrolled over two register sets), so every figure is divided by the number of pairs: "per
iteration" means per pair of lines, as in the source.

Classes (by mnemonic, so that the script stays a count and not a data-flow analysis):
  moves       v_mov_b32 / v_pk_mov_b32 / v_accvgpr_* whose source is a VGPR or a literal (copies, re-materialised constants)
  address     integer VALU: v_mov_b32 from an SGPR, integer add / shift / mad, v_cmp_*_{i,u}32, and v_cndmask_b32 with a
              literal 0 source (the clamped row index of the parent commit); the `m < i` tests of use0 / use1 count here
  selects     v_cmp_*_f32 (incl. class tests) and every other v_cndmask_b32: parallel tests, sign tests, interval updates
  arithmetic  everything else (v_pk_mul / add / fma, v_mul / add / fma, v_rcp_f32)
"""
import argparse
import re

FLAGSHIP = "ca_pipe_kernelILi10ELi4ELb1ELb1ELb0ELb0ELb0E"


def kernel_body(lines, sub):
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and sub in l and l.rstrip().split(":")[0].endswith("KArgsE"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start:end + 1]


def loops(body):
    """-> {header label: [instruction lines]} for the inner loops of the kernel"""
    out, cur, own = {}, None, None
    for l in body:
        if re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):", l):      # a block starts: which loop does its comment name?
            own = l[2:].split(":")[0] if l.startswith(".LBB") else None
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
            cur = h.group(1) if h else (own if "Inner Loop Header" in l else None)
        elif l.lstrip().startswith(";"):                       # (a header's comment runs over several lines)
            if "Inner Loop Header" in l and own:
                cur = own
        elif cur and re.match(r"^\s+(v_|s_|ds_|buffer_|global_|flat_)", l):
            out.setdefault(cur, []).append(l.strip())
    return out


def classify(ins):
    op, _, rest = ins.partition(" ")
    args = [a.strip() for a in rest.split(";")[0].split(",")]
    if op.startswith(("v_mov_b32", "v_pk_mov_b32", "v_accvgpr")):
        return "address" if any(re.match(r"^s\d+$|^s\[", a) for a in args[1:]) else "moves"
    if re.match(r"v_cmpx?_\w+_[iu](32|16|64)", op):
        return "address"
    if op.startswith("v_cmp"):
        return "selects"
    if op.startswith("v_cndmask"):
        return "address" if "0" in args[1:3] else "selects"
    if re.match(r"v_(add|sub|subrev|lshl|lshlrev|lshrrev|ashrrev|mad|mul_lo|mul_hi|mul_u32|mul_i32|and|or|xor|lshl_add|add_lshl|lshl_or|add3|min|max)_?\w*[iub](16|24|32|64)", op):
        return "address"
    return "arithmetic"


def census(path, sub):
    body = kernel_body(open(path).read().split("\n"), sub)
    rows = []
    for h, ins in loops(body).items():
        v = [i for i in ins if i.startswith("v_")]
        rcp = sum(i.startswith("v_rcp_f32") for i in v)
        other = sum(i.startswith(("v_sqrt", "v_rsq", "v_rcp_f64", "v_exp", "v_log", "v_sin", "v_cos")) for i in v)
        lds = sum(i.startswith("ds_read") for i in ins)
        if rcp < 2 or rcp % 2 or other or not lds:
            continue
        pairs = rcp // 2
        c = {"moves": 0, "address": 0, "selects": 0, "arithmetic": 0}
        for i in v:
            c[classify(i.split(";")[0])] += 1
        rows.append({"header": h, "pairs_per_trip": pairs, "valu_per_trip": len(v), "lds_reads_per_trip": lds,
                     "salu_per_trip": sum(i.startswith("s_") and not i.startswith(("s_nop", "s_waitcnt")) for i in ins),
                     "per_iteration": {k: n / pairs for k, n in c.items()}, "valu_per_iteration": len(v) / pairs, "text": ins})
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default=FLAGSHIP)
    ap.add_argument("--list", action="store_true", help="print the instructions of each loop")
    a = ap.parse_args()
    for r in census(a.asm, a.kernel):
        p = r["per_iteration"]
        print("loop %-10s pairs/trip %d  VALU/iteration %5.1f  (moves %.1f, address %.1f, selects %.1f, arithmetic %.1f)  LDS reads/trip %d  SALU/trip %d"
              % (r["header"], r["pairs_per_trip"], r["valu_per_iteration"], p["moves"], p["address"], p["selects"], p["arithmetic"],
                 r["lds_reads_per_trip"], r["salu_per_trip"]))
        if a.list:
            print("    " + "\n    ".join(r["text"]))
