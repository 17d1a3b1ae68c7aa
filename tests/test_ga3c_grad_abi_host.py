"""The ABI of the network's backward pass (include/cagpu.h, "GRADIENTS OF THE GA3C-CADRL NETWORK"), without a GPU: the
three symbols are exported by the built library, the two host-only calls answer, and the ctypes mirror of CaNetGrad has
the header's size and offsets (the addition leaves CAGPU_VERSION at 12)."""
import ctypes
import os
import re

from gym_collision_avoidance_amd import _native as nat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_host_only_calls():
    lib = nat.lib()
    for n in ("cagpu_ga3c_grad_floats", "cagpu_ga3c_grad_work_bytes", "cagpu_ga3c_grad"):
        assert n in nat.EXPORTS and hasattr(lib, n)
    assert lib.cagpu_ga3c_grad.restype is ctypes.c_int
    assert nat.ABI_VERSION == 12 and lib.cagpu_version() == 12
    assert int(lib.cagpu_ga3c_grad_floats()) == 170764
    assert int(lib.cagpu_ga3c_grad_work_bytes(-1)) == 0 and int(lib.cagpu_ga3c_grad_work_bytes(1 << 31)) == 0
    a, b = int(lib.cagpu_ga3c_grad_work_bytes(1000)), int(lib.cagpu_ga3c_grad_work_bytes(2000))
    assert 0 < a < b and a % 4 == 0


def test_struct_mirror():
    P = ctypes.sizeof(ctypes.c_void_p)
    S = nat.CaNetGrad
    assert ctypes.sizeof(S) == 9 * P + 8 + 4 + 4 == 88
    assert [n for n, _ in S._fields_] == ["x", "rows", "width", "accumulate", "live", "dlogits", "dvalue", "value_kernel",
                                          "value_bias", "grad", "work", "work_bytes"]
    assert (S.rows.offset, S.width.offset, S.accumulate.offset, S.live.offset) == (8, 16, 20, 24)
    assert (S.grad.offset, S.work.offset, S.work_bytes.offset) == (64, 72, 80)
    header = open(os.path.join(REPO, "include", "cagpu.h")).read()
    assert re.search(r"#define CAGPU_VERSION 12\b", header)
    body = re.search(r"typedef struct CaNetGrad \{(.*?)\} CaNetGrad;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?\s*(\w+)\s*[,;]", body)
    assert names == [n for n, _ in S._fields_], names
    for decl in ("uint64_t cagpu_ga3c_grad_floats(void);", "uint64_t cagpu_ga3c_grad_work_bytes(int64_t rows);",
                 "int cagpu_ga3c_grad(const CaNet *net, const CaNetGrad *g, void *stream);"):
        assert decl in header
