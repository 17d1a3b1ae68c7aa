"""The backward pass of the GA3C-CADRL graph (test infrastructure; no test file by itself): the judge of cagpu_ga3c_grad.

  grad               a hand-written float64 NumPy backward of ga3c_f64_ref.evaluate -- back-propagation through the 19 masked
                     LSTM steps, the three ReLU layers and both heads -- for upstream gradients on the logits and the value;
                     with want_abs also sum_b |gradient of row b| per tensor, the denominator of the accuracy measure
  torch_forward      the same graph restated in torch (any dtype, CPU): float64 autograd holds `grad` to its purpose
                     (tests/test_ga3c_grad_host.py), float32 autograd is the yardstick e32 of the GPU test
  torch_grad         its autograd gradient for the same upstream gradients
  a3c_loss / a3c_loss_grad   ga3c_train.a3c_loss in float64 NumPy and its closed-form gradient
  descent_problem    the 256-row problem of the descent tests

The reference ships no training code for this network: there is nothing to compare with but the graph itself."""
import numpy as np

from tests import ga3c_f64_ref as f64

NO, HID = f64.NUM_OTHERS, f64.HIDDEN
LAYOUT = (("lstm_kernel", (71, 256)), ("lstm_bias", (256,)), ("layer1_kernel", (68, 256)), ("layer1_bias", (256,)),
          ("layer2_kernel", (256, 256)), ("layer2_bias", (256,)), ("fc1_kernel", (256, 256)), ("fc1_bias", (256,)),
          ("logits_p_kernel", (256, 11)), ("logits_p_bias", (11,)), ("logits_v_kernel", (256, 1)), ("logits_v_bias", (1,)))
KEYS = tuple(k for k, _ in LAYOUT)
TOTAL = 170764


def offsets():
    """-> {key: (offset, shape)} of the flat gradient"""
    out, at = {}, 0
    for k, s in LAYOUT:
        out[k] = (at, s)
        at += int(np.prod(s))
    return out


def _inputs(w, x, live):
    """-> (lv [B] bool, seq [B] 0..19 (0 where not live), host [B,4], others [B,19,7] float64, zero at and behind the length
    and in rows that are not live: nothing there is ever read)"""
    x = np.asarray(x, dtype=np.float32)
    B = x.shape[0]
    lv = np.ones(B, bool) if live is None else np.asarray(live).reshape(B) != 0
    xs = np.where(lv[:, None], x, np.float32(0))
    if xs.shape[1] < f64.INPUT_LEN:
        xs = np.concatenate([xs, np.zeros((B, f64.INPUT_LEN - xs.shape[1]), np.float32)], axis=1)
    xs = xs[:, :f64.INPUT_LEN]
    with np.errstate(invalid="ignore"):
        cnt = np.where(np.isfinite(xs[:, 0]), xs[:, 0], 0)
    seq = np.clip(np.trunc(np.clip(cnt, -100, 100)), 0, NO).astype(np.int64) * lv
    slot_live = np.arange(NO)[None, :] < seq[:, None]
    clean = xs.copy()
    clean[:, 5:] = np.where(np.repeat(slot_live, 7, axis=1), xs[:, 5:], np.float32(0))
    clean[:, 0] = 0
    xn = f64.normalise(w, clean).astype(np.float64)
    others = xn[:, 5:].reshape(B, NO, 7) * slot_live[..., None]
    host = xn[:, 1:5] * lv[:, None]
    return lv, seq, host, others


def _sg(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def grad(w, x, dlogits=None, dvalue=None, live=None, want_abs=False):
    """-> {key: float64 gradient}: the sum over the live rows of the row's vector-Jacobian product (the value head's two
    entries are zeros without dvalue).  want_abs: -> (gradient, {key: sum_b |gradient of row b|})."""
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    lv, seq, host, others = _inputs(w, x, live)
    B = lv.shape[0]
    # ---- forward, keeping what the backward pass needs
    h, c = np.zeros((B, HID)), np.zeros((B, HID))
    ins, gates, cs, cprevs = [], [], [], []
    for t in range(NO):
        a_in = np.concatenate([others[:, t], h], axis=1)
        z = a_in @ W["lstm_kernel"] + W["lstm_bias"]
        zi, zj, zf, zo = np.split(z, 4, axis=1)
        i, j, f, o = _sg(zi), np.tanh(zj), _sg(zf + 1.0), _sg(zo)
        cn = f * c + i * j
        hn = o * np.tanh(cn)
        m = (t < seq)[:, None]
        ins.append(a_in); gates.append((i, j, f, o)); cprevs.append(c); cs.append(cn)
        c, h = np.where(m, cn, c), np.where(m, hn, h)
    a0 = np.concatenate([host, h], axis=1)
    a1 = np.maximum(a0 @ W["layer1_kernel"] + W["layer1_bias"], 0)
    a2 = np.maximum(a1 @ W["layer2_kernel"] + W["layer2_bias"], 0)
    a3 = np.maximum(a2 @ W["fc1_kernel"] + W["fc1_bias"], 0)
    # ---- backward
    dzp = np.zeros((B, 11)) if dlogits is None else np.asarray(dlogits, np.float64).reshape(B, 11) * lv[:, None]
    dzv = np.zeros((B, 1)) if dvalue is None else np.asarray(dvalue, np.float64).reshape(B, 1) * lv[:, None]
    if dvalue is not None and "logits_v_kernel" not in W:
        raise ValueError("dvalue needs a value head")
    wv = W["logits_v_kernel"] if "logits_v_kernel" in W else np.zeros((256, 1))
    g, ab = {}, {}

    def dense(name, a, dz):
        g[name + "_kernel"], g[name + "_bias"] = a.T @ dz, dz.sum(axis=0)
        ab[name + "_kernel"], ab[name + "_bias"] = np.abs(a).T @ np.abs(dz), np.abs(dz).sum(axis=0)
    dense("logits_p", a3, dzp)
    dense("logits_v", a3, dzv)
    dz3 = (dzp @ W["logits_p_kernel"].T + dzv @ wv.T) * (a3 > 0)
    dense("fc1", a2, dz3)
    dz2 = (dz3 @ W["fc1_kernel"].T) * (a2 > 0)
    dense("layer2", a1, dz2)
    dz1 = (dz2 @ W["layer2_kernel"].T) * (a1 > 0)
    dense("layer1", a0, dz1)
    dh, dc = (dz1 @ W["layer1_kernel"].T)[:, 4:], np.zeros((B, HID))
    dzs = [None] * NO
    for t in range(NO - 1, -1, -1):
        i, j, f, o = gates[t]
        m = (t < seq)[:, None]
        tc = np.tanh(cs[t])
        dct = dc + dh * o * (1.0 - tc * tc)
        dz = np.concatenate([dct * j * i * (1.0 - i), dct * i * (1.0 - j * j), dct * cprevs[t] * f * (1.0 - f),
                             dh * tc * o * (1.0 - o)], axis=1) * m
        dzs[t] = dz
        dh = np.where(m, dz @ W["lstm_kernel"][7:].T, dh)
        dc = np.where(m, dct * f, dc)
    A, Z = np.stack(ins, axis=1), np.stack(dzs, axis=1)          # [B, 19, 71], [B, 19, 256]
    g["lstm_kernel"] = np.einsum("btk,btn->kn", A, Z)
    g["lstm_bias"] = Z.sum(axis=(0, 1))
    if not want_abs:
        return g
    ak, abias = np.zeros((71, 256)), np.zeros(256)
    for b0 in range(0, B, 64):
        ak += np.abs(np.einsum("btk,btn->bkn", A[b0:b0 + 64], Z[b0:b0 + 64])).sum(axis=0)
        abias += np.abs(Z[b0:b0 + 64].sum(axis=1)).sum(axis=0)
    ab["lstm_kernel"], ab["lstm_bias"] = ak, abias
    return g, ab


def flat(g):
    """{key: array} -> the flat [170764] gradient in LAYOUT's order"""
    return np.concatenate([np.asarray(g[k], np.float64).reshape(-1) for k in KEYS])


# ---------------------------------------------------------------- the graph in torch
def torch_forward(wt, w, x, live=None):
    """wt: {key: torch tensor (CPU, any float dtype)}; w: the numpy weights (for the float32 normalisation); -> (logits
    [B, 11], value [B]) in wt's dtype.  The inputs are the ones `grad` uses (_inputs)."""
    import torch
    dt = wt["lstm_kernel"].dtype
    lv, seq, host, others = _inputs(w, x, live)
    B = lv.shape[0]
    host, others = torch.as_tensor(host, dtype=dt), torch.as_tensor(others, dtype=dt)
    seq_t = torch.as_tensor(seq)
    h, c = torch.zeros((B, HID), dtype=dt), torch.zeros((B, HID), dtype=dt)
    for t in range(NO):
        z = torch.cat([others[:, t], h], dim=1) @ wt["lstm_kernel"] + wt["lstm_bias"]
        zi, zj, zf, zo = torch.split(z, HID, dim=1)
        cn = torch.sigmoid(zf + 1.0) * c + torch.sigmoid(zi) * torch.tanh(zj)
        hn = torch.sigmoid(zo) * torch.tanh(cn)
        m = (t < seq_t)[:, None]
        c, h = torch.where(m, cn, c), torch.where(m, hn, h)
    a = torch.cat([host, h], dim=1)
    for n in ("layer1", "layer2", "fc1"):
        a = torch.relu(a @ wt[n + "_kernel"] + wt[n + "_bias"])
    return a @ wt["logits_p_kernel"] + wt["logits_p_bias"], (a @ wt["logits_v_kernel"] + wt["logits_v_bias"])[:, 0]


def torch_grad(w, x, dlogits=None, dvalue=None, live=None, dtype="float64"):
    """autograd's gradient of sum(dlogits * logits) + sum(dvalue * value) over the live rows -> {key: numpy float64}"""
    import torch
    dt = getattr(torch, dtype)
    wt = {k: torch.tensor(np.asarray(w[k]), dtype=dt, requires_grad=True) for k in KEYS}
    logits, value = torch_forward(wt, w, x, live)
    B = logits.shape[0]
    lv = torch.as_tensor(np.ones(B, bool) if live is None else np.asarray(live).reshape(B) != 0)
    loss = torch.zeros((), dtype=dt)
    if dlogits is not None:
        loss = loss + (torch.as_tensor(np.asarray(dlogits), dtype=dt).reshape(B, 11) * logits)[lv].sum()
    if dvalue is not None:
        loss = loss + (torch.as_tensor(np.asarray(dvalue), dtype=dt).reshape(B) * value)[lv].sum()
    loss.backward()
    return {k: (np.zeros(wt[k].shape) if wt[k].grad is None else wt[k].grad.numpy().astype(np.float64)) for k in KEYS}


# ---------------------------------------------------------------- the objective
def a3c_loss(logits, value, action, advantage, returns, beta=0.01, value_coef=0.5, temperature=1.0):
    """ga3c_train.a3c_loss in float64 NumPy, averaged over all rows"""
    z = np.asarray(logits, np.float64) / temperature
    z = z - z.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    ent = -(p * logp).sum(axis=1)
    lp = logp[np.arange(z.shape[0]), np.asarray(action)]
    per = -(advantage * lp) - beta * ent + value_coef * 0.5 * (returns - np.asarray(value, np.float64)) ** 2
    return per.mean()


def a3c_loss_grad(logits, value, action, advantage, returns, beta=0.01, value_coef=0.5, temperature=1.0):
    """the closed form of d a3c_loss / d logits [B, 11] and / d value [B]:
    (-advantage (onehot - p) + beta p (logp + H)) / (temperature B),  value_coef (value - returns) / B"""
    z = np.asarray(logits, np.float64) / temperature
    B = z.shape[0]
    z = z - z.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    H = -(p * logp).sum(axis=1, keepdims=True)
    onehot = np.zeros_like(p)
    onehot[np.arange(B), np.asarray(action)] = 1.0
    adv = np.asarray(advantage, np.float64)[:, None]
    dl = (-adv * (onehot - p) + beta * p * (logp + H)) / (temperature * B)
    dv = value_coef * (np.asarray(value, np.float64) - returns) / B
    return dl, dv


def descent_problem():
    """the descent tests' problem: 256 plausible rows under np.random.default_rng(5), random actions, N(0,1) advantages and
    returns -> (x float32 [256,138], action int64, advantage, returns float64)"""
    from tests import ga3c_edge_rows as er
    rng = np.random.default_rng(5)
    x = er.plausible_x(rng, rng.integers(0, NO + 1, 256))
    action = rng.integers(0, 11, 256)
    return x, action, rng.standard_normal(256), rng.standard_normal(256)


DESCENT_LR, DESCENT_STEPS = 1e-3, 5


def descent_loss(w, prob):
    x, action, adv, ret = prob
    logits, value, _ = f64.evaluate(w, x)
    return a3c_loss(logits, value, action, adv, ret)


def descent_reference(w, prob, lr=DESCENT_LR, steps=DESCENT_STEPS):
    """plain SGD in float64 on the reference gradient -> the losses [steps + 1]"""
    x, action, adv, ret = prob
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    w32 = {"input_mean": np.asarray(w["input_mean"], np.float32), "input_std": np.asarray(w["input_std"], np.float32)}
    losses = []
    for s in range(steps + 1):
        ww = dict(w, **w32)
        logits, value, _ = _evaluate64(ww, x)
        losses.append(a3c_loss(logits, value, action, adv, ret))
        if s == steps:
            break
        dl, dv = a3c_loss_grad(logits, value, action, adv, ret)
        g = grad(ww, x, dl, dv)
        for k in KEYS:
            w[k] = w[k] - lr * g[k]
    return losses


def _evaluate64(w, x):
    """f64.evaluate without its float32 cast of the weights' dict (the weights stay float64 between SGD steps)"""
    return f64.evaluate(w, x)
