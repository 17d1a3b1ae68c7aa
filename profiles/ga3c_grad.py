"""What the weight gradients of the GA3C-CADRL network cost: one cagpu_ga3c_grad call (its launches between two device
events) at 81 920 and 5 120 rows, core.ga3c_grad under its default 256 MB workspace budget (chunked at 81 920 rows), and the
path a user has without it -- the graph restated in torch, a float32 forward pass and autograd's backward on the same GPU
and rows.  Warm-up first; every figure is the median over `--blocks` blocks of `--reps` calls each, with the spread
(min .. max of the block means).  Prints one JSON line per figure.

    python profiles/ga3c_grad.py [--blocks 7] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from gym_collision_avoidance_amd import _native as nat  # noqa: E402
from gym_collision_avoidance_amd import core  # noqa: E402

NO = 19


def rows_like_a_batch(rng, n):
    """plausible policy vectors: counts 0..19, the first `count` slots filled (tests/ga3c_edge_rows.plausible_x's ranges)"""
    num = rng.integers(0, NO + 1, n)
    x = np.zeros((n, 138), np.float32)
    x[:, 0] = num
    x[:, 1] = rng.uniform(0.1, 12.0, n)
    x[:, 2] = rng.uniform(-np.pi, np.pi, n)
    x[:, 3] = rng.uniform(0.5, 1.5, n)
    x[:, 4] = rng.uniform(0.2, 0.8, n)
    lo = np.array([-8, -8, -1.5, -1.5, 0.2, 0.4, 0.0], np.float32)
    hi = np.array([8, 8, 1.5, 1.5, 0.8, 1.6, 10.0], np.float32)
    slots = rng.uniform(lo, hi, (n, NO, 7)).astype(np.float32)
    x[:, 5:] = (slots * (np.arange(NO)[None, :] < num[:, None])[..., None]).reshape(n, 7 * NO)
    return x


def timed(fn, blocks, reps):
    """-> (median, min, max) of the block means, milliseconds per call, by device events"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    means = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        means.append(a.elapsed_time(b) / reps)
    return float(np.median(means)), float(min(means)), float(max(means))


def torch_graph(wt, x, dtype=torch.float32):
    """the graph in torch on the device (float32, or float64 behind the float32 normalisation): -> (logits, value)"""
    mean, std = wt["input_mean"], wt["input_std"]
    seq = x[:, 0].to(torch.int32).clamp(0, NO)
    xn = ((x - mean.to(x.dtype)) / std.to(x.dtype)).to(dtype)
    host, others = xn[:, 1:5], xn[:, 5:].reshape(-1, NO, 7)
    B = x.shape[0]
    h = torch.zeros((B, 64), device=x.device, dtype=dtype)
    c = torch.zeros((B, 64), device=x.device, dtype=dtype)
    for t in range(NO):
        z = torch.cat([others[:, t], h], dim=1) @ wt["lstm_kernel"] + wt["lstm_bias"]
        zi, zj, zf, zo = torch.split(z, 64, dim=1)
        cn = torch.sigmoid(zf + 1.0) * c + torch.sigmoid(zi) * torch.tanh(zj)
        hn = torch.sigmoid(zo) * torch.tanh(cn)
        m = (t < seq)[:, None]
        c, h = torch.where(m, cn, c), torch.where(m, hn, h)
    a = torch.cat([host, h], dim=1)
    for n in ("layer1", "layer2", "fc1"):
        a = torch.relu(a @ wt[n + "_kernel"] + wt[n + "_bias"])
    return a @ wt["logits_p_kernel"] + wt["logits_p_bias"], (a @ wt["logits_v_kernel"] + wt["logits_v_bias"])[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="*", default=[81920, 5120])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profiles/ga3c_grad.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    L = nat.lib()
    rng = np.random.default_rng(2024)
    net, ts, _ = core._query_net(None, dev)
    with np.load(core.GA3C_DEFAULT_WEIGHTS) as z:
        wnp = {k: z[k].astype(np.float32) for k in z.files}
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for rows in args.rows:
        x = torch.from_numpy(rows_like_a_batch(rng, rows)).to(dev)
        dl = torch.from_numpy(rng.standard_normal((rows, 11)).astype(np.float32)).to(dev)
        dv = torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).to(dev)
        work = torch.empty((int(L.cagpu_ga3c_grad_work_bytes(rows)),), dtype=torch.uint8, device=dev)
        flat = torch.empty((int(L.cagpu_ga3c_grad_floats()),), dtype=torch.float32, device=dev)
        q = nat.CaNetGrad(x=x.data_ptr(), rows=rows, width=138, accumulate=0, live=None, dlogits=dl.data_ptr(),
                          dvalue=dv.data_ptr(), value_kernel=ts["value_kernel"].data_ptr(),
                          value_bias=ts["value_bias"].data_ptr(), grad=flat.data_ptr(), work=work.data_ptr(),
                          work_bytes=work.numel())
        one = lambda: nat.check(L.cagpu_ga3c_grad(C.byref(net), C.byref(q), st))
        med, lo, hi = timed(one, args.blocks, args.reps)
        print(json.dumps(dict(what="cagpu_ga3c_grad, one call", rows=rows, ms=med, ms_min=lo, ms_max=hi,
                              work_bytes=work.numel(), kernel=L.cagpu_last_kernel().decode())), flush=True)
        del work
        chunk = core.ga3c_grad_chunk_rows(rows, 256 << 20)
        med, lo, hi = timed(lambda: core.ga3c_grad(x, dl, dv), args.blocks, args.reps)
        print(json.dumps(dict(what="core.ga3c_grad, 256 MB budget", rows=rows, chunk_rows=chunk, ms=med, ms_min=lo,
                              ms_max=hi)), flush=True)
        ours = core.ga3c_grad(x, dl, dv)
        # the path a user has today: the graph in torch, float32, forward + autograd
        wt = {k: torch.from_numpy(v).to(dev).requires_grad_(not k.startswith("input_")) for k, v in wnp.items()}
        params = [v for v in wt.values() if v.requires_grad]

        def torch_path():
            for p in params:
                p.grad = None
            logits, value = torch_graph(wt, x)
            ((dl * logits).sum() + (dv * value).sum()).backward()
        med, lo, hi = timed(torch_path, args.blocks, args.reps)
        print(json.dumps(dict(what="torch float32 forward + autograd", rows=rows, ms=med, ms_min=lo, ms_max=hi)), flush=True)
        fwd = lambda: torch_graph(wt, x)
        with torch.no_grad():
            med, lo, hi = timed(fwd, args.blocks, args.reps)
        print(json.dumps(dict(what="torch float32 forward alone", rows=rows, ms=med, ms_min=lo, ms_max=hi)), flush=True)
        # both float32 gradients against a float64 autograd evaluation on the device: |g - g64|_F / |g64|_F per tensor
        # (g64 itself cancels between rows under N(0,1) upstream gradients: the figure is large for both, compare the two)
        torch_path()
        w64 = {k: torch.from_numpy(v).to(dev).to(torch.float64 if not k.startswith("input_") else torch.float32)
               .requires_grad_(not k.startswith("input_")) for k, v in wnp.items()}
        logits, value = torch_graph(w64, x, torch.float64)
        ((dl.double() * logits).sum() + (dv.double() * value).sum()).backward()
        rel = lambda g, k: float((g.double().reshape(w64[k].shape) - w64[k].grad).norm() / w64[k].grad.norm())
        print(json.dumps(dict(what="|g - g64|_F / |g64|_F, worst tensor", rows=rows,
                              ours=max(rel(ours[k], k) for k in ours),
                              torch_float32=max(rel(wt[k].grad, k) for k in ours))), flush=True)
        del w64, logits, value
        del x, dl, dv, flat, wt, params, ours
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
