"""The GA3C-CADRL network as a torch module whose forward AND backward pass are the project's own kernels: the network that
acts (cagpu_ga3c_query / ga3c_kernel) and the network that learns (cagpu_ga3c_grad) are one statement of the graph, and
collect -> gae -> loss -> backward -> optimiser -> BatchedSim.update_ga3c never leaves the device.

The reference ships no training code for this network: `a3c_loss` is THIS PROJECT's statement of the A3C objective (policy
gradient with an advantage, an entropy bonus, a squared value error), written for the sampler's rule (log-softmax of
logits / temperature)."""
import ctypes as C

import numpy as np
import torch

from . import _native as nat
from . import core

PARAMS = tuple(k for k, _ in core.GA3C_GRAD_LAYOUT)
_TO_FIELD = {v: k for k, v in core._GA3C_NAMES.items()}      # checkpoint key -> CaNet field where the two differ


class _Network(torch.autograd.Function):
    """(logits, value) = network(x); backward: ONE cagpu_ga3c_grad call for both heads"""

    @staticmethod
    def forward(ctx, module, x, live, *params):
        ctx.module, ctx.x, ctx.live = module, x, live
        ctx.set_materialize_grads(False)
        out = module._query(x)
        ctx.versions = module._versions()      # the parameters this forward pass saw
        return out

    @staticmethod
    def backward(ctx, dlogits, dvalue):
        m = ctx.module
        if dlogits is None and dvalue is None:
            return (None,) * (3 + len(PARAMS))
        if m._versions() != ctx.versions:
            raise RuntimeError("TrainableGA3C: a parameter was modified in place between the forward and the backward pass "
                               "(the gradient is recomputed from the parameters: it would be another network's)")
        flat = torch.empty((core.ga3c_grad_offsets()[None][0],), dtype=torch.float32, device=ctx.x.device)
        cont = lambda t: None if t is None else t.to(torch.float32).contiguous()
        core._ga3c_grad_into(flat, m._canet(), m.logits_v_kernel.data, m.logits_v_bias.data, ctx.x, cont(dlogits),
                             cont(dvalue), ctx.live, m.max_work_bytes)      # (no pack: the gradient reads the plain weights)
        views = core.ga3c_grad_views(flat)
        return (None, None, None) + tuple(views[k] for k in PARAMS)


class TrainableGA3C(torch.nn.Module):
    """The GA3C-CADRL network with the checkpoint's keys and shapes as parameters (lstm_kernel ... logits_v_bias;
    input_mean / input_std are buffers), on one GPU.  weights: None (the shipped default), an .npz path, or a dict of
    arrays / tensors with the checkpoint's keys; a value head (logits_v_*) is required.

    forward(x, live=None) -> (logits [rows, 11], value [rows]) runs cagpu_ga3c_query on the CURRENT parameters: the weights
    are packed for the matrix cores again only when a parameter's version counter has moved since the last pack (`packs`
    counts them).  Rows with live == 0 are evaluated like the others by the forward pass (their results are whatever their
    x gives: mask them, as a3c_loss does) and never read by the backward pass.  backward: cagpu_ga3c_grad, once for both
    heads; parameters' .grad are views of one flat buffer until autograd accumulates."""

    def __init__(self, weights=None, device="cuda:0", max_work_bytes=256 << 20):
        super().__init__()
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        if weights is None:
            weights = core.GA3C_DEFAULT_WEIGHTS
        if isinstance(weights, str):
            with np.load(weights) as z:
                weights = {k: z[k] for k in z.files}
        shapes = dict(core.GA3C_GRAD_LAYOUT, input_mean=(138,), input_std=(138,))
        for k, shape in shapes.items():
            if k not in weights:
                raise ValueError("TrainableGA3C: the weights lack %s" % k)
            v = weights[k]
            v = v.detach().clone() if torch.is_tensor(v) else torch.from_numpy(np.array(v, dtype=np.float32))
            v = v.to(device=device, dtype=torch.float32).contiguous()
            if tuple(v.shape) != shape:
                raise ValueError("TrainableGA3C: %s has shape %s, expected %s" % (k, tuple(v.shape), shape))
            if k.startswith("input_"):
                self.register_buffer(k, v)
            else:
                self.register_parameter(k, torch.nn.Parameter(v))
        self.max_work_bytes = int(max_work_bytes)
        self.packs = 0
        self._packed = torch.empty((int(nat.lib().cagpu_ga3c_packed_bytes()),), dtype=torch.uint8, device=device)
        self._packed_at = None

    @classmethod
    def load(cls, sim, index=0, **kw):
        """a module that starts from the network a BatchedSim has loaded at `index` (load_ga3c(keep_value=True))"""
        if int(index) not in sim._nets:
            raise nat.CagpuError("TrainableGA3C.load: no GA3C-CADRL checkpoint loaded at index %s" % index)
        ts = sim._nets[int(index)][1]
        if "value_kernel" not in ts:
            raise ValueError("TrainableGA3C.load: the loaded checkpoint has no value head")
        w = {core._GA3C_NAMES.get(f, f): ts[f] for f in nat.NET_FIELDS}
        w["logits_v_kernel"], w["logits_v_bias"] = ts["value_kernel"].reshape(256, 1), ts["value_bias"]
        return cls(w, device=sim.device, **kw)

    def _versions(self):
        return tuple((getattr(self, k).data_ptr(), getattr(self, k)._version) for k in PARAMS + ("input_mean", "input_std"))

    def _canet(self):
        """a CaNet over the parameters' own memory (packed: the module's buffer, whatever it holds)"""
        return nat.CaNet(packed=self._packed.data_ptr(),
                         **{f: getattr(self, core._GA3C_NAMES.get(f, f)).data_ptr() for f in nat.NET_FIELDS})

    def _net(self):
        """-> (the CaNet, its planes packed again where a parameter changed; True if it packed)"""
        net = self._canet()
        now = self._versions()
        if now == self._packed_at:
            return net, False
        dev = self._packed.device
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            nat.check(nat.lib().cagpu_ga3c_pack(C.byref(net), self._packed.data_ptr(), self._packed.numel(), st))
        self._packed_at = now
        self.packs += 1
        return net, True

    def _query(self, x):
        net, _ = self._net()
        rows = int(x.shape[0])
        logits = torch.empty((rows, 11), dtype=torch.float32, device=x.device)
        value = torch.empty((rows,), dtype=torch.float32, device=x.device)
        if rows:
            q = nat.CaNetQuery(x=x.data_ptr(), rows=rows, width=int(x.shape[1]), value_kernel=self.logits_v_kernel.data_ptr(),
                               value_bias=self.logits_v_bias.data_ptr(), logits=logits.data_ptr(), value=value.data_ptr(),
                               action=None)
            with torch.cuda.device(x.device):
                st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
                nat.check(nat.lib().cagpu_ga3c_query(C.byref(net), C.byref(q), st))
        return logits, value

    def forward(self, x, live=None):
        dev = self._packed.device
        x = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] < 1:
            raise ValueError("TrainableGA3C: x must be [rows, width >= 1], got shape %s" % (tuple(x.shape),))
        if live is not None:
            live = torch.as_tensor(live).to(dev).contiguous()
            live = live.view(torch.uint8) if live.dtype == torch.bool else live.to(torch.uint8)
            if tuple(live.shape) != (int(x.shape[0]),):
                raise ValueError("TrainableGA3C: live must be [rows]")
        return _Network.apply(self, x.detach(), live, *[getattr(self, k) for k in PARAMS])

    def tensors(self):
        """-> {checkpoint key: the parameter's (or buffer's) tensor}: what BatchedSim.update_ga3c takes"""
        return {k: getattr(self, k).detach() for k in PARAMS + ("input_mean", "input_std")}


def a3c_loss(logits, value, action, advantage, returns, live=None, beta=0.01, value_coef=0.5, temperature=1.0):
    """This project's statement of the A3C objective (the reference ships none), plain torch on [rows, 11] tensors:

        -(advantage * logp(action)) - beta * entropy + value_coef * 1/2 (returns - value)^2

    averaged over the live rows (all rows without `live`; 0 when no row is live), logp = log_softmax(logits / temperature)
    -- the sampler's rule (CaGa3cSample) -- and entropy = -sum p logp.  advantage and returns are constants (detached).
    Rows that are not live are masked by selection, not by a product: what the network gave for them (NaN included) does not
    reach the loss or its gradient."""
    rows = logits.shape[0]
    action = action.reshape(rows).long()
    advantage, returns = advantage.reshape(rows).detach(), returns.reshape(rows).detach()
    if live is not None:
        live = live.reshape(rows).bool()
        logits = torch.where(live[:, None], logits, torch.zeros_like(logits))
        value = torch.where(live, value.reshape(rows), torch.zeros_like(value.reshape(rows)))
    logp = torch.log_softmax(logits / temperature, dim=-1)
    entropy = -(logp.exp() * logp).sum(dim=-1)
    if live is not None:
        action = torch.where(live, action, torch.zeros_like(action))     # (a slot that is not live holds no action)
    lp = logp.gather(1, action[:, None])[:, 0]      # (an index outside 0..10 in a live row is an error, as in torch.gather)
    per = -(advantage * lp) - beta * entropy + value_coef * 0.5 * (returns - value.reshape(rows)) ** 2
    if live is None:
        return per.mean() if rows else per.sum()
    per = torch.where(live, per, torch.zeros_like(per))
    return per.sum() / live.sum().clamp(min=1).to(per.dtype)
