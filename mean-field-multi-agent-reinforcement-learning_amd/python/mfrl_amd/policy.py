"""QNetHIP: the hand-written HIP forward (csrc/policy_kernels.hip, csrc/qnet_bf16_kernels.hip) of the reference's
Q network.

    ValueNet._construct_net  examples/battle_model/algo/base.py:123-183   -> QNetHIP.forward (q values)
    ValueNet.act             examples/battle_model/algo/base.py:228-254   -> QNetHIP.act (argmax q)

The weights come from a torch QNet (mfrl_amd.algo.nets, the layer-for-layer port that training updates):
``load(qnet)`` packs them into the device layout the kernels read -- every matrix [K][N] row-major with
the im2col / NHWC-flatten orders of TF (conv kernels [ky][kx][ci][co], Dense-Obs rows in (y, x, c) order),
K padded to a multiple of 4 with zero rows -- and uploads them in one copy.  Forward only: training keeps
the torch module (autograd); after an optimiser step call ``load`` again.

Numerics, precision="f32" (the default): f32 inputs and weights, f32 MFMA accumulation (one rounding per
product); the result differs from the torch module's by summation order only (|dq| ~1e-6 at these sizes,
tests/test_policy_gpu.py).

precision="bf16" (opt-in, acting only): the operands of every matrix product -- the weights, the inputs and
each layer's activation after bias and ReLU -- are rounded to bf16 (nearest even); products accumulate in f32,
biases and ReLU stay f32, the Q values are written unrounded.  The Q values then differ from the f32 ones by
the quantisation error (a few 1e-3 of the Q scale, tests/test_policy_bf16_cpu.py), so the greedy action can
differ where the top two Q values are that close.  The contract is stated in csrc/qnet_bf16_kernels.hip and
restated in numpy in tests/qnet_bf16_ref.py.

temperature=T on forward / act / act_rollout (opt-in; None, the default, is the reference's greedy act): the action is
drawn from softmax(q / T) in the same kernels' epilogue, in both precisions -- the contract of csrc/qsample.h (f32
weights expf((q - max q) / T), a running-sum draw against the actor-critic draw's counter-hash uniform), restated in
numpy in tests/qsample_ref.py.  The Q values are the greedy call's bit for bit.

ACNetHIP: the actor-critic network (ActorCritic / MFAC, algo/ac.py) on csrc/acnet_kernels.hip, the same two modes.
precision="bf16" is the policy path only -- view, feature, dense 512, x / 0.1, policy, the draw -- on
csrc/acnet_bf16_kernels.hip: the four weight matrices, the view and feature inputs, h_view and h_emb after bias and
ReLU, and relu(d) / 0.1 (the exact f32 division, then one rounding) go into the products as bf16; accumulation (from
the f32 bias), ReLU, softmax, the clip and the draw are f32, the draw's rule and uniforms unchanged.  A policy entry
then moves by about 1e-2 at most (the division by 0.1 amplifies the error; tests/test_acnet_bf16_cpu.py), which a
sampling policy tolerates and a bootstrap value would not: forward(want_value=True) raises in this mode, and the
input support, which the f32 kernel uses bit-identically, is not used.  The contract is restated in numpy in
tests/acnet_bf16_ref.py.

RuleHIP (at the end): the scripted rush / random opponent on csrc/rule_kernels.hip -- no network, one action per
observation row; the rule is restated in numpy in tests/rule_ref.py.
"""
import ctypes

import numpy as np

import torch

from . import check, lib
from .abi import ptr, stream


def rows_scratch(E, rowcap):
    """Ints of the act_rollout row-list scratch: E * rowcap rows, the row count, one total per 64-env chunk
    (include/magent_amd.h, mfx_qnet_act_rollout)."""
    return E * rowcap + 1 + (E + 63) // 64


def _rollout_args(scratch, eng, group, names):
    """What an act_rollout call reads of engine `eng`: the pointers of its rollout buffers `names` (the group's view
    and feature, the batch's counts, mean actions and actions) and the row-list scratch (rows pointer, total pointer).
    The scratch, rows_scratch(E, rowcap) ints, is kept in the dict `scratch` per engine, so engines on different
    streams may share one network."""
    E, rc = eng.n_envs, eng.rowcap
    rows = scratch.get(id(eng))
    if rows is None or rows.numel() < rows_scratch(E, rc):
        rows = scratch[id(eng)] = torch.empty(rows_scratch(E, rc), dtype=torch.int32, device="cuda")
    bufs = {name: eng.rollout_buffer(name, group if name in ("view", "feature") else 0) for name in names}
    return bufs, rows.data_ptr(), rows.data_ptr() + 4 * E * rc


def _record_event(ts):
    ev = torch.cuda.Event()
    ev.record(ts)
    return ev


class StreamOrder:
    """Which streams have seen a handle's current device state (DESIGN "streams").  The contract it keeps for QNetHIP /
    ACNetHIP: after load, set_blob, set_precision or set_input_support returns, a later forward / act_rollout of that
    handle on *any* stream reads the new state.  (Only that direction: an upload does not wait for act kernels still
    pending on another stream that read the state it overwrites -- synchronise those before uploading, as the shipped
    loops do with finish().)

    produced(sid, ts): state was enqueued on stream `ts` (id `sid`: its hipStream_t).  A new generation begins; only
    that stream has seen it.  ready(sid, ts): make the state visible on stream `sid` -- at a stream's first use in a
    generation an event is recorded on the producer's stream (once per generation, and only if a foreign stream ever
    asks) and the consumer's stream waits for it.  After that, and always for the producer's own stream, the call is a
    set lookup: no event is recorded or waited for.  A producer that reads the state it extends (the support image
    gathers from the blob) calls ready() for its own stream first, so the order is transitive.
    record(stream) -> event and wait(stream, event) are torch's by default; tests pass fakes."""

    def __init__(self, record=_record_event, wait=lambda ts, ev: ts.wait_event(ev)):
        self.gen = 0
        self.seen = set()           # stream ids ordered after the current generation's producer
        self._producer = None       # the stream object the current generation was enqueued on
        self._event = None          # recorded on it, at the first foreign consumer
        self._record, self._wait = record, wait

    def produced(self, sid, ts):
        self.gen += 1
        self._producer, self._event = ts, None
        self.seen = {sid}

    def ready(self, sid, ts):
        """-> True when stream `sid` had to wait.  ts: the stream object, or a callable giving it (called only then)."""
        if sid in self.seen or self._producer is None:
            return False
        if self._event is None:
            self._event = self._record(self._producer)
        self._wait(ts() if callable(ts) else ts, self._event)
        self.seen.add(sid)
        return True


PRECISIONS = {"f32": 0, "bf16": 1}      # mfx_qnet_set_precision / mfx_acnet_set_precision

N_BLOCKS = 18      # w1 b1 w2 b2 wd bd we be wp1 bp1 wp2 bp2 w2d b2d wo bo wq bq (policy_kernels.hip)


def blob_layout(feature, n_action, use_mf):
    """(floats in the packed blob, the 18 block offsets) -- mfx_qnet_blob_size (host only, no GPU)."""
    n = ctypes.c_size_t()
    off = (ctypes.c_size_t * N_BLOCKS)()
    check(lib().mfx_qnet_blob_size(int(feature), int(n_action), int(bool(use_mf)), ctypes.byref(n), off),
          "mfx_qnet_blob_size")
    return n.value, list(off)


def pack_qnet(net, feature, n_action, use_mf, layout=None):
    """The device-layout blob (float32, on net's device) of a torch QNet (mfrl_amd.algo.nets.QNet)."""
    F, A, mf = int(feature), int(n_action), bool(use_mf)
    n, offsets = layout or blob_layout(F, A, mf)
    Fp, Ap = (F + 3) & ~3, (A + 3) & ~3
    dev = net.conv1.weight.device
    blob = torch.zeros(n, dtype=torch.float32, device=dev)

    def put(k, mat, rows=None, cols=None):
        m = mat.detach().to(torch.float32)
        if m.dim() == 1:
            blob[offsets[k]:offsets[k] + m.numel()] = m
            return
        R, C = m.shape
        R2, C2 = rows or R, cols or C
        full = torch.zeros((R2, C2), dtype=torch.float32, device=dev)
        full[:R, :C] = m
        blob[offsets[k]:offsets[k] + R2 * C2] = full.reshape(-1)

    put(0, net.conv1.weight.permute(2, 3, 1, 0).reshape(-1, 32), rows=64)       # [ky][kx][ci][co]
    put(1, net.conv1.bias)
    put(2, net.conv2.weight.permute(2, 3, 1, 0).reshape(-1, 32))
    put(3, net.conv2.bias)
    put(4, net.dense_obs.weight.t())                                          # [2592 (y, x, c)][256]
    put(5, net.dense_obs.bias)
    put(6, net.dense_emb.weight.t(), rows=Fp)
    put(7, net.dense_emb.bias)
    if mf:
        put(8, net.prob_emb.weight.t(), rows=Ap)
        put(9, net.prob_emb.bias)
        put(10, net.dense_act_prob.weight.t())
        put(11, net.dense_act_prob.bias)
    put(12, net.dense2.weight.t())
    put(13, net.dense2.bias)
    put(14, net.dense_out.weight.t())
    put(15, net.dense_out.bias)
    put(16, net.q_value.weight.t(), cols=32)                                  # Q columns padded to 32
    put(17, net.q_value.bias)
    return blob


@torch.no_grad()
def unpack_qnet(blob, net, feature=None, n_action=None, use_mf=None, layout=None):
    """The inverse of pack_qnet: the blob's 18 blocks copied in place (copy_) into the parameters of torch QNet `net`
    (padding rows / columns dropped).  blob: float32 tensor on any device; the shapes default to the net's own."""
    F = int(net.dense_emb.in_features if feature is None else feature)
    A = int(net.q_value.out_features if n_action is None else n_action)
    mf = bool(net.use_mf if use_mf is None else use_mf)
    n, offsets = layout or blob_layout(F, A, mf)
    assert blob.numel() == n, "unpack_qnet: %d floats, the layout has %d" % (blob.numel(), n)
    Fp, Ap = (F + 3) & ~3, (A + 3) & ~3

    def mat(k, rows, cols):
        return blob[offsets[k]:offsets[k] + rows * cols].reshape(rows, cols)

    def vec(k, p):
        p.copy_(blob[offsets[k]:offsets[k] + p.numel()])

    def dense(k, layer, rows=None, cols=None):
        out_f, in_f = layer.weight.shape
        layer.weight.copy_(mat(k, rows or in_f, cols or out_f)[:in_f, :out_f].t())
        vec(k + 1, layer.bias)

    net.conv1.weight.copy_(mat(0, 64, 32)[:63].reshape(3, 3, -1, 32).permute(3, 2, 0, 1))
    vec(1, net.conv1.bias)
    net.conv2.weight.copy_(mat(2, 288, 32).reshape(3, 3, 32, 32).permute(3, 2, 0, 1))
    vec(3, net.conv2.bias)
    dense(4, net.dense_obs)
    dense(6, net.dense_emb, rows=Fp)
    if mf:
        dense(8, net.prob_emb, rows=Ap)
        dense(10, net.dense_act_prob)
    dense(12, net.dense2)
    dense(14, net.dense_out)
    dense(16, net.q_value, cols=32)
    return net


class QNetHIP:
    def __init__(self, view_space, feature_space, num_actions, use_mf=False, precision="f32"):
        if precision not in PRECISIONS:
            raise ValueError("QNetHIP: precision %r (one of %s)" % (precision, ", ".join(PRECISIONS)))
        self.precision = precision
        h, w, c = view_space
        self.F, self.A, self.use_mf = int(feature_space[0]), int(num_actions), bool(use_mf)
        self._L = L = lib()
        self.blob_n, self.offsets = blob_layout(self.F, self.A, self.use_mf)
        hdl = ctypes.c_void_p()
        check(L.mfx_qnet_create(int(h), int(w), int(c), self.F, self.A, int(self.use_mf), ctypes.byref(hdl)),
              "mfx_qnet_create")
        self.handle = hdl
        self._rows = {}
        self._order = StreamOrder()
        if precision != "f32":
            check(L.mfx_qnet_set_precision(hdl, PRECISIONS[precision], None), "mfx_qnet_set_precision")

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self._L.mfx_qnet_destroy(self.handle)
            self.handle = None

    def pack(self, net):
        return pack_qnet(net, self.F, self.A, self.use_mf, (self.blob_n, self.offsets))

    def load(self, net):
        """Upload the weights of torch QNet `net` (same shapes), on the current stream.  Every later forward /
        act_rollout of this handle, on any stream, reads them (StreamOrder)."""
        self._blob = self.pack(net).contiguous()
        sid = stream()
        check(self._L.mfx_qnet_set_weights(self.handle, ptr(self._blob), self.blob_n, sid), "mfx_qnet_set_weights")
        self._order.produced(sid, torch.cuda.current_stream())
        return self

    # ------------------------------------------------------------------ forward
    def forward(self, view, feature, prob=None, want_q=True, temperature=None, seed=0, step=0, want_w=False):
        """view [n, 13, 13, 7], feature [n, F], prob [n, A] (mean field) float32 CUDA tensors ->
        (q [n, A] float32 or None, actions [n] int32 = argmax q).

        temperature (the opt-in Boltzmann mode; None: greedy, the call above): row i's action is drawn from the weights
        expf((q - max q) / temperature) with the uniform (seed, step, group 0, row i) -- the contract of csrc/qsample.h,
        restated in tests/qsample_ref.py; q is what the greedy call gives.  want_w: the weights [n, A] float32 as a
        third result.  A temperature that is not finite and > 0 raises (nothing is launched)."""
        if temperature is None and want_w:
            raise ValueError("QNetHIP.forward: want_w needs a temperature")
        sid = stream()
        if sid not in self._order.seen:                 # (the weights were uploaded on another stream)
            self._order.ready(sid, torch.cuda.current_stream)
        n = view.shape[0]
        view = view.reshape(n, -1).contiguous().float()
        feature = feature.reshape(n, -1).contiguous().float()
        if self.use_mf:
            assert prob is not None and prob.shape[0] == n
            prob = prob.reshape(n, -1).contiguous().float()
        q = torch.empty((n, self.A), dtype=torch.float32, device=view.device) if want_q else None
        act = torch.empty(n, dtype=torch.int32, device=view.device)
        if temperature is not None:
            w = torch.empty((n, self.A), dtype=torch.float32, device=view.device) if want_w else None
            check(self._L.mfx_qnet_forward_sample(self.handle, ptr(view), ptr(feature),
                                                  ptr(prob if self.use_mf else None), int(n), ptr(q), ptr(w), ptr(act),
                                                  temperature, seed, step, sid), "mfx_qnet_forward_sample")
            return (q, act, w) if want_w else (q, act)
        check(self._L.mfx_qnet_forward(self.handle, ptr(view), ptr(feature), ptr(prob if self.use_mf else None),
                                       int(n), ptr(q), ptr(act), sid), "mfx_qnet_forward")
        return q, act

    def act(self, view, feature, prob=None, temperature=None, seed=0, step=0):
        return self.forward(view, feature, prob, want_q=False, temperature=temperature, seed=seed, step=step)[1]

    def act_rollout(self, eng, group, temperature=None, seed=0, step=0, prob_rows=None):
        """Actions of group `group` of a BattleBatch rollout from its current observation buffers and
        former mean actions, written into the rollout's action buffer [E][G][rowcap] (live rows only).
        temperature (None: greedy): the Boltzmann draw of forward(), row j of env e with the uniform
        (seed, step, group, e * rowcap + j).
        prob_rows (None: the rollout's mean action of the env, one row per (env, group)): a float32 CUDA tensor
        [E, rowcap, A], contiguous -- row j of env e reads its own mean action prob_rows[e, j] (the neighbourhood mean,
        mfrl_amd.mf.NeighborMean.rows); it must be ready on the engine's stream.

        Streams: the kernels run on the engine's stream.  The weights may have been uploaded (load) on any other
        stream: the engine's stream waits for that upload the first time it uses the handle afterwards -- every engine
        that shares the handle does, each once per upload (StreamOrder); later calls, and an engine on the uploading
        stream, wait for nothing.  The observation buffers and prob_rows are the caller's to order.

        Works on every plan that takes a learned policy (BattleBatch.rollout_policy_path: all but
        MFX_ROLLOUT_PIPE=1 -- large batches, large envs and few-env batches alike; E, rowcap and the buffers come
        from the engine; the row-list scratch is per engine, so engines on different streams may share this network).
        The observation must be current: call eng.rollout_policy_observe() after rollout_init,
        rollout_step or any per-call API use, before the first act_rollout / rollout_policy_step pair."""
        E, rc, G = eng.n_envs, eng.rowcap, len(eng.handles)
        buf, rows, total = _rollout_args(self._rows, eng, group,
                                         ("view", "feature", "group_num", "mean_action", "actions"))
        if prob_rows is not None:
            if (prob_rows.dtype != torch.float32 or not prob_rows.is_cuda or not prob_rows.is_contiguous()
                    or tuple(prob_rows.shape) != (E, rc, self.A)):
                raise ValueError("QNetHIP.act_rollout: prob_rows must be a contiguous float32 CUDA tensor [%d, %d, %d], "
                                 "got %s %s" % (E, rc, self.A, prob_rows.dtype, tuple(prob_rows.shape)))
            prob = (ptr(prob_rows),)
        else:
            prob = (buf["mean_action"], int(eng.mean_stride()))
        args = (self.handle, buf["view"], buf["feature"], buf["group_num"], *prob, int(E), int(G), int(group), int(rc),
                rows, total, buf["actions"])
        if temperature is not None:
            args += (temperature, seed, step)
        sid = eng.stream_handle()
        if sid not in self._order.seen:
            self._order.ready(sid, eng.torch_stream)
        fn = {(False, False): "mfx_qnet_act_rollout", (False, True): "mfx_qnet_act_rollout_sample",
              (True, False): "mfx_qnet_act_rollout_rows", (True, True): "mfx_qnet_act_rollout_rows_sample"}[
                  (prob_rows is not None, temperature is not None)]
        check(getattr(self._L, fn)(*args, sid), fn)


# ---------------------------------------------------------------------------------------------------------------
# the actor-critic network (ActorCritic / MFAC, algo/ac.py:48-98, :219-276) on csrc/acnet_kernels.hip
# ---------------------------------------------------------------------------------------------------------------
AC_BLOCKS = 19     # wv bv we be wd0 wd1 bd wp bp wval bval wep bep wdp bdp wvd bvd wvo bvo (acnet_kernels.hip)


def acnet_layout(view_floats, feature, n_action, use_mf):
    """(floats in the packed blob, the 19 block offsets) -- mfx_acnet_blob_size (host only, no GPU)."""
    n = ctypes.c_size_t()
    off = (ctypes.c_size_t * AC_BLOCKS)()
    check(lib().mfx_acnet_blob_size(int(view_floats), int(feature), int(n_action), int(bool(use_mf)), ctypes.byref(n),
                                    off), "mfx_acnet_blob_size")
    return n.value, list(off)


def pack_acnet(net, view_floats, feature, n_action, use_mf, layout=None):
    """The device-layout blob (float32, on net's device) of a torch ACNet (mfrl_amd.algo.nets.ACNet)."""
    V, F, A, mf = int(view_floats), int(feature), int(n_action), bool(use_mf)
    n, offsets = layout or acnet_layout(V, F, A, mf)
    Vp, Fp, Ap = (V + 3) & ~3, (F + 3) & ~3, (A + 3) & ~3
    dev = net.h_view.weight.device
    blob = torch.zeros(n, dtype=torch.float32, device=dev)

    def put(k, mat, rows=None, cols=None):
        m = mat.detach().to(torch.float32)
        if m.dim() == 1:
            blob[offsets[k]:offsets[k] + m.numel()] = m
            return
        R, C = m.shape
        full = torch.zeros((rows or R, cols or C), dtype=torch.float32, device=dev)
        full[:R, :C] = m
        blob[offsets[k]:offsets[k] + full.numel()] = full.reshape(-1)

    put(0, net.h_view.weight.t(), rows=Vp)                    # [V (NHWC flatten)][256]
    put(1, net.h_view.bias)
    put(2, net.h_emb.weight.t(), rows=Fp)
    put(3, net.h_emb.bias)
    wd = net.dense.weight.t()                                 # [512 in][512 out], by output halves
    put(4, wd[:, :256])
    put(5, wd[:, 256:])
    put(6, net.dense.bias)
    put(7, net.policy.weight.t(), cols=32)
    put(8, net.policy.bias)
    if mf:
        put(11, net.emb_prob.weight.t(), rows=Ap)
        put(12, net.emb_prob.bias)
        put(13, net.dense_prob.weight.t())
        put(14, net.dense_prob.bias)
        put(15, net.value_dense.weight.t())                   # [544 = concat 512 + dense_prob 32][256]
        put(16, net.value_dense.bias)
        put(17, net.value.weight.t(), cols=16)
        put(18, net.value.bias)
    else:
        put(9, net.value.weight.t(), cols=16)
        put(10, net.value.bias)
    return blob


def _acnet_blocks(net, V, F, A, mf):
    """(block, layer, rows, cols) of every dense layer of a torch ACNet in the blob: the weight block [rows][cols]
    holds the layer's weight^T in its top-left corner, the next block its bias."""
    Vp, Fp, Ap = (V + 3) & ~3, (F + 3) & ~3, (A + 3) & ~3
    out = [(0, net.h_view, Vp, 256), (2, net.h_emb, Fp, 256), (7, net.policy, 512, 32)]
    if mf:
        out += [(11, net.emb_prob, Ap, 64), (13, net.dense_prob, 64, 32), (15, net.value_dense, 544, 256),
                (17, net.value, 256, 16)]
    else:
        out += [(9, net.value, 512, 16)]
    return out


@torch.no_grad()
def unpack_acnet(blob, net, view_floats=None, feature=None, n_action=None, use_mf=None, layout=None, into=None):
    """The inverse of pack_acnet: the blob's blocks copied in place (copy_) into the parameters of torch ACNet `net`
    (padding rows / columns dropped).  blob: float32 tensor on any device; the shapes default to the net's own.
    into: a list of tensors shaped like net.parameters(), in their order, filled instead of the parameters (a gradient
    blob -> per-parameter gradients); `net` then only gives the shapes."""
    V = int(net.h_view.in_features if view_floats is None else view_floats)
    F = int(net.h_emb.in_features if feature is None else feature)
    A = int(net.policy.out_features if n_action is None else n_action)
    mf = bool(net.use_mf if use_mf is None else use_mf)
    n, offsets = layout or acnet_layout(V, F, A, mf)
    assert blob.numel() == n, "unpack_acnet: %d floats, the layout has %d" % (blob.numel(), n)
    dst = {id(p): t for p, t in zip(net.parameters(), into)} if into is not None else None

    def out(p):
        return p if dst is None else dst[id(p)]

    def mat(k, rows, cols):
        return blob[offsets[k]:offsets[k] + rows * cols].reshape(rows, cols)

    for k, layer, rows, cols in _acnet_blocks(net, V, F, A, mf):
        out_f, in_f = layer.weight.shape
        out(layer.weight).copy_(mat(k, rows, cols)[:in_f, :out_f].t())
        out(layer.bias).copy_(blob[offsets[k + 1]:offsets[k + 1] + out_f])
    out(net.dense.weight).copy_(torch.cat([mat(4, 512, 256), mat(5, 512, 256)], dim=1).t())
    out(net.dense.bias).copy_(blob[offsets[6]:offsets[6] + 512])
    return net if into is None else into


class ACNetHIP:
    """Forward of ActorCritic / MFAC on the HIP kernel k_acnet: the clipped softmax policy, the value, and the
    draw of tf.multinomial(log(policy)) from a counter-hash uniform (seed, step, group, row).  precision="bf16":
    the policy and the draw from bf16 matrix operands (acting only: no value; the module docstring)."""

    def __init__(self, view_space, feature_space, num_actions, use_mf=False, precision="f32"):
        if precision not in PRECISIONS:
            raise ValueError("ACNetHIP: precision %r (one of %s)" % (precision, ", ".join(PRECISIONS)))
        self.precision = precision
        V = 1
        for d in view_space:
            V *= int(d)
        self.V, self.F, self.A, self.use_mf = V, int(feature_space[0]), int(num_actions), bool(use_mf)
        self._L = L = lib()
        self.blob_n, self.offsets = acnet_layout(self.V, self.F, self.A, self.use_mf)
        hdl = ctypes.c_void_p()
        check(L.mfx_acnet_create(self.V, self.F, self.A, int(self.use_mf), ctypes.byref(hdl)), "mfx_acnet_create")
        self.handle = hdl
        self._rows = {}
        self._support = None
        self._order = StreamOrder()
        if precision != "f32":
            check(L.mfx_acnet_set_precision(hdl, PRECISIONS[precision], None), "mfx_acnet_set_precision")

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self._L.mfx_acnet_destroy(self.handle)
            self.handle = None

    def pack(self, net):
        return pack_acnet(net, self.V, self.F, self.A, self.use_mf, (self.blob_n, self.offsets))

    def load(self, net):
        """Upload the weights of torch ACNet `net` (same shapes), on the current stream.  Every later forward /
        act_rollout of this handle, on any stream, reads them (StreamOrder)."""
        self._blob = self.pack(net).contiguous()
        return self._upload()

    def _upload(self):
        sid = stream()
        check(self._L.mfx_acnet_set_weights(self.handle, ptr(self._blob), self.blob_n, sid), "mfx_acnet_set_weights")
        self._order.produced(sid, torch.cuda.current_stream())
        return self

    def set_blob(self, blob):
        """Set the weights from a packed blob on the device (pack_acnet's layout; e.g. ACTrainHIP's parameters):
        a device-to-device copy, no packing."""
        assert blob.is_cuda and blob.dtype == torch.float32 and blob.numel() == self.blob_n
        self._blob = blob.contiguous()
        return self._upload()

    def set_precision(self, precision):
        """Switch the handle's mode (mfx_acnet_set_precision): the f32 weights stay, the images the mode lacks are
        built on the current stream, so no re-upload is needed and f32 results are the same before and after."""
        if precision not in PRECISIONS:
            raise ValueError("ACNetHIP: precision %r (one of %s)" % (precision, ", ".join(PRECISIONS)))
        if precision != self.precision:
            sid = self._extend()
            check(self._L.mfx_acnet_set_precision(self.handle, PRECISIONS[precision], sid), "mfx_acnet_set_precision")
            self._order.produced(sid, torch.cuda.current_stream())
            self.precision = precision
        return self

    def _extend(self):
        """The current stream's id, ordered after the handle's state: what a call that builds images from the weights
        (a mode's first images, the support image) starts with, before it becomes the state's producer itself."""
        sid = stream()
        if sid not in self._order.seen:
            self._order.ready(sid, torch.cuda.current_stream)
        return sid

    def set_input_support(self, mask):
        """mask: uint8/bool [V], 1 where the view can be non-zero (e.g. BattleBatch.view_support), or None for the
        dense order.  Later forwards run the view layer over the supported inputs only -- the same results bit for
        bit while the view is zero elsewhere, which the caller guarantees (the engine's observation buffers are)."""
        if mask is None:
            check(self._L.mfx_acnet_set_input_support(self.handle, None, 0, stream()), "mfx_acnet_set_input_support")
            self._support = None
            return self
        m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint8).reshape(-1))
        sid = self._extend()
        try:
            check(self._L.mfx_acnet_set_input_support(self.handle, ptr(m), int(m.size), sid),
                  "mfx_acnet_set_input_support")
        except Exception:
            # a mask of the wrong size leaves the handle and self._support as they were; a support whose packed chunks
            # span too far is refused with the old one already freed: the handle is back on the dense order
            if self.input_support_size() == 0:
                self._support = None
            raise
        self._order.produced(sid, torch.cuda.current_stream())
        self._support = m.copy()
        return self

    def input_support_size(self):
        """Inputs the view layer runs over (0: the dense order)."""
        k = ctypes.c_int()
        check(self._L.mfx_acnet_input_support_size(self.handle, ctypes.byref(k)), "mfx_acnet_input_support_size")
        return k.value

    def forward(self, view, feature, prob=None, want_policy=True, want_value=False, want_act=True, seed=0, step=0):
        """view [n, ...] (flattened to V), feature [n, F], prob [n, A] (the MF value head) float32 CUDA tensors
        -> (policy [n, A] or None, value [n] or None, actions [n] int32 or None; row i drawn with (seed, step,
        group 0, row i)).  precision="bf16" is acting only: want_value raises ValueError."""
        if want_value and self.precision != "f32":
            raise ValueError("ACNetHIP: precision %r is acting only (no value head)" % self.precision)
        sid = self._extend()
        n = view.shape[0]
        view = view.reshape(n, -1).contiguous().float()
        feature = feature.reshape(n, -1).contiguous().float()
        if want_value and self.use_mf:
            assert prob is not None and prob.shape[0] == n
            prob = prob.reshape(n, -1).contiguous().float()
        else:
            prob = None
        dev = view.device
        pol = torch.empty((n, self.A), dtype=torch.float32, device=dev) if want_policy else None
        val = torch.empty(n, dtype=torch.float32, device=dev) if want_value else None
        act = torch.empty(n, dtype=torch.int32, device=dev) if want_act else None
        check(self._L.mfx_acnet_forward(self.handle, ptr(view), ptr(feature), ptr(prob), int(n), ptr(pol), ptr(val),
                                        ptr(act), seed, step, sid), "mfx_acnet_forward")
        return pol, val, act

    def act(self, view, feature, seed=0, step=0):
        return self.forward(view, feature, want_policy=False, seed=seed, step=step)[2]

    def act_rollout(self, eng, group, seed, step, support=True):
        """Sampled actions of group `group` of a BattleBatch rollout from its current observation buffers,
        written into the rollout's action buffer [E][G][rowcap] (live rows; row j of env e drawn with (seed,
        step, group, e * rowcap + j)).  Nothing is read back to the host.  support: run the view layer over the
        inputs the engine's view can make non-zero only (BattleBatch.view_support; bit-identical).  The row-list
        scratch is per engine, so engines on different streams may share this network.

        Streams: the kernels run on the engine's stream.  The weights, a mode's images and the support image --
        built by this very call, on the current stream, when the support is not the handle's yet -- may come from any
        other stream: the engine's stream waits for them the first time it uses the handle afterwards, every engine
        that shares the handle each once (StreamOrder); later calls, and an engine on the producing stream, wait for
        nothing."""
        E, rc, G = eng.n_envs, eng.rowcap, len(eng.handles)
        if support:
            m = eng.view_support(group)
            if self._support is None or not np.array_equal(self._support, m):
                self.set_input_support(m)
        elif self._support is not None:
            self.set_input_support(None)
        buf, rows, total = _rollout_args(self._rows, eng, group, ("view", "feature", "group_num", "actions"))
        sid = eng.stream_handle()
        if sid not in self._order.seen:
            self._order.ready(sid, eng.torch_stream)
        check(self._L.mfx_acnet_act_rollout(self.handle, buf["view"], buf["feature"], buf["group_num"], int(E), int(G),
                                            int(group), int(rc), rows, total, buf["actions"], seed, step, sid),
              "mfx_acnet_act_rollout")


# ---------------------------------------------------------------------------------------------------------------
# the scripted opponents "rush" / "random" (mfrl_amd.algo.rule) on csrc/rule_kernels.hip
# ---------------------------------------------------------------------------------------------------------------
class RuleHIP:
    """The scripted rule of csrc/rule_kernels.hip (k_rule_act; restated in tests/rule_ref.py): one action
    per observation row from that row alone -- attack the first attackable enemy, else step toward the nearest enemy
    in view, else toward the densest enemy bin of the minimap, else toward the map's centre; with probability eps a
    uniform action.  The handle is pure data (the type's view2attack and move tables), made on the host: constructing
    one needs no GPU, and one handle serves the host loops (act) and every rollout plan that takes a learned policy
    (act_rollout)."""

    def __init__(self, view_space, feature_space, num_actions, attack_base, view2attack, move_delta):
        h, w, c = (int(x) for x in view_space)
        self.view_space, self.V = (h, w, c), h * w * c
        self.F, self.A = int(feature_space[0]), int(num_actions)
        self._L = L = lib()
        v2a = np.ascontiguousarray(np.asarray(view2attack, dtype=np.int32).reshape(-1))
        mv = np.asarray(move_delta, dtype=np.int32).reshape(-1, 2)
        if v2a.size != h * w:
            raise ValueError("RuleHIP: view2attack has %d cells, the view %d x %d" % (v2a.size, h, w))
        if len(mv) != int(attack_base):
            raise ValueError("RuleHIP: %d moves, attack_base %d (turn mode is not supported)" % (len(mv), attack_base))
        dx, dy = np.ascontiguousarray(mv[:, 0]), np.ascontiguousarray(mv[:, 1])
        shape = (ctypes.c_int32 * 4)(h, w, c, self.F)
        hdl = ctypes.c_void_p()
        check(L.mfx_rule_create(shape, int(attack_base), self.A, ptr(v2a), ptr(dx), ptr(dy), ctypes.byref(hdl)),
              "mfx_rule_create")
        self.handle = hdl
        self._rows = {}

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self._L.mfx_rule_destroy(self.handle)
            self.handle = None

    def act(self, view, feature, eps=0.0, seed=0, step=0, group=0):
        """view [n, VH, VW, 7], feature [n, F] float32 CUDA tensors -> actions [n] int32; row i's exploration draw
        uses the uniform (seed, step, group, i).  An eps outside [0, 1] raises (nothing is launched)."""
        n = view.shape[0]
        if view.numel() != n * self.V or feature.numel() != n * self.F:
            raise ValueError("RuleHIP.act: %d rows of %s view and %s feature floats, the handle takes %d and %d"
                             % (n, tuple(view.shape[1:]), tuple(feature.shape[1:]), self.V, self.F))
        view = view.reshape(n, self.V).contiguous().float()
        feature = feature.reshape(n, self.F).contiguous().float()
        if not 0.0 <= eps <= 1.0:
            raise ValueError("RuleHIP.act: eps must be in [0, 1], got %r" % (eps,))
        act = torch.empty(n, dtype=torch.int32, device=view.device)
        if n:
            check(self._L.mfx_rule_act(self.handle, ptr(view), ptr(feature), int(n), eps, seed, step, int(group),
                                       ptr(act), stream()), "mfx_rule_act")
        return act

    def act_rollout(self, eng, group, eps=0.0, seed=0, step=0):
        """Actions of group `group` of a BattleBatch rollout from its current observation buffers, written into the
        rollout's action buffer [E][G][rowcap] (live rows only; row j of env e drawn with (seed, step, group,
        e * rowcap + j)).  Nothing is read back.  Runs on every plan that takes a learned policy; the row-list scratch
        is per engine."""
        E, rc, G = eng.n_envs, eng.rowcap, len(eng.handles)
        buf, rows, total = _rollout_args(self._rows, eng, group, ("view", "feature", "group_num", "actions"))
        check(self._L.mfx_rule_act_rollout(self.handle, buf["view"], buf["feature"], buf["group_num"], int(E), int(G),
                                           int(group), int(rc), rows, total, buf["actions"], eps, seed, step,
                                           eng.stream_handle()), "mfx_rule_act_rollout")
