"""The numpy statement of the GA3C-CADRL network's value head (test infrastructure; no test file by itself): the hidden
layers exactly as oracle/ga3c_ref.GA3CNet.logits computes them (input normalisation, the LSTM over the first
num_other_agents slots, layer1 / layer2 / fullyconnected1 with ReLU), then `logits_v` -- one column, `Squeeze:0` of the
graph (GA3C_CADRL/network.py:74).  float32 throughout, summation order numpy's.  tests/test_ga3c_query_host.py holds it to
tests/golden/ga3c_value.npz (the checkpoints' own graphs) at atol 2e-6."""
import numpy as np

from oracle.ga3c_ref import HIDDEN, INPUT_LEN, NUM_OTHERS, GA3CNet, _sigmoid


def crop_x(x):
    """[B, width] -> [B, 138] float32: cut / zero-pad (network.py:24-35)"""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros((x.shape[0], INPUT_LEN), dtype=np.float32)
    n = min(INPUT_LEN, x.shape[1])
    out[:, :n] = x[:, :n]
    return out


def hidden(net, x):
    """X [B,138] float32 -> the activations of fullyconnected1 [B,256] (the lines of GA3CNet.logits up to its last)"""
    w = net.w
    x = np.asarray(x, dtype=np.float32)
    B = x.shape[0]
    seq = x[:, 0].astype(np.int32)
    xn = ((x - w["input_mean"]) / w["input_std"]).astype(np.float32)
    host = xn[:, 1:5]
    others = xn[:, 5:].reshape(B, NUM_OTHERS, 7)
    h = np.zeros((B, HIDDEN), np.float32)
    c = np.zeros((B, HIDDEN), np.float32)
    for t in range(NUM_OTHERS):
        z = np.concatenate([others[:, t], h], axis=1) @ w["lstm_kernel"] + w["lstm_bias"]
        i, j, f, o = np.split(z.astype(np.float32), 4, axis=1)
        c_new = _sigmoid(f + np.float32(1.0)) * c + _sigmoid(i) * np.tanh(j)
        h_new = _sigmoid(o) * np.tanh(c_new)
        live = (t < seq)[:, None]
        c = np.where(live, c_new, c).astype(np.float32)
        h = np.where(live, h_new, h).astype(np.float32)
    a = np.concatenate([host, h], axis=1)
    a = np.maximum(a @ w["layer1_kernel"] + w["layer1_bias"], 0).astype(np.float32)
    a = np.maximum(a @ w["layer2_kernel"] + w["layer2_bias"], 0).astype(np.float32)
    return np.maximum(a @ w["fc1_kernel"] + w["fc1_bias"], 0).astype(np.float32)


def logits_and_value(net, x):
    """-> (logits_p/BiasAdd [B,11], Squeeze [B]) of a GA3CNet on X [B,138]"""
    a = hidden(net, x)
    w = net.w
    logits = (a @ w["logits_p_kernel"] + w["logits_p_bias"]).astype(np.float32)
    value = (a @ w["logits_v_kernel"] + w["logits_v_bias"]).astype(np.float32)[:, 0]
    return logits, value


def value(net, x):
    return logits_and_value(net, x)[1]


def softmax(l):
    e = np.exp(l - l.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


__all__ = ["GA3CNet", "crop_x", "hidden", "logits_and_value", "value", "softmax"]
