"""Operator cost model for the search (reference Simulator::measure_operator_cost,
src/runtime/simulator.cu:58 — profiles each op with per-shard shapes on GPU 0, warmup 5 /
repeat 10 — plus the hard-coded ~2019-GPU machine constants of machine_model.cc:67-69).

Two sources, same interface (`op_cost(layer, cfg) -> (fwd_ms, bwd_ms, mem_bytes)`):
  * measured: run the op's real forward+backward (our HIP kernels) on the local GPU with the
    per-part shard shapes of the config; cached per (op, attributes, shard shapes) so BERT's 24
    identical layers cost one measurement per distinct config;
  * analytic: an MI355X roofline — MFMA ops at a shape-dependent fraction of the 2.5 PF/s dense
    bf16 peak (tile wave-quantization over 256 CUs), memory-bound ops at ~5.5 TB/s HBM3E.
"""
from __future__ import annotations

import math
import os
import time
from typing import Dict, Tuple

import torch

from ..parallel.layout import Layout
from ..type import DataType, OperatorType
from .strategy import OpConfig, op_layouts

PEAK_BF16 = 2.5e15
PEAK_FP32 = 1.5e14
HBM = 5.5e12
LAUNCH_S = 4e-6

_measured: Dict[tuple, Tuple[float, float]] = {}

# Measured costs persist in a JSON table keyed by repr(cost key) and the device name, so every
# search in a process, and every process that loads the same table, prices an op identically (r5:
# two passes over the same 8-way DP plan priced it 8.55 vs 7.31 ms, each timing every op once).
# FF_COST_CACHE=path reads and extends that table; without it the table shipped with the package
# (measured on MI355X by scripts/gpu_cost_table.sh) is read, never written. FF_COST_CACHE=0: off.
_SHIPPED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "op_costs_mi355x.json")
_disk = {"path": None, "table": None, "dirty": False}
STATS = {"table_hits": 0, "timed": 0, "timed_s": 0.0}  # this process's measured-cost lookups


def _cache_path():
    p = os.environ.get("FF_COST_CACHE")
    if p == "0":
        return None, False
    return (p, True) if p else (_SHIPPED, False)


def _dev_tag(device) -> str:
    try:
        return torch.cuda.get_device_name(device)
    except Exception:
        return "?"


def _disk_table():
    path, _ = _cache_path()
    if path is None:
        return {}
    if _disk["table"] is None or _disk["path"] != path:
        tab = {}
        if os.path.exists(path):
            import json
            try:
                with open(path) as f:
                    tab = json.load(f).get("costs", {})
            except (OSError, ValueError):
                tab = {}
        _disk.update(path=path, table=tab, dirty=False)
    return _disk["table"]


def _disk_get(key, device):
    e = _disk_table().get(repr(key))
    if e is not None and e.get("device") == _dev_tag(device):
        return float(e["fwd_ms"]), float(e["bwd_ms"])
    return None


def _disk_put(key, device, tf, tb):
    path, writable = _cache_path()
    if path is None or not writable:
        return
    _disk_table()[repr(key)] = {"device": _dev_tag(device), "fwd_ms": round(tf, 5), "bwd_ms": round(tb, 5)}
    _disk["dirty"] = True


def save_cost_table():
    """Write the measured-cost table (FF_COST_CACHE) if this process added entries."""
    path, writable = _cache_path()
    if not (writable and _disk["dirty"]):
        return None
    import json
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        json.dump({"format": "flexflow_amd op costs v1", "costs": _disk["table"]}, f, indent=0, sort_keys=True)
    os.replace(tmp, path)
    _disk["dirty"] = False
    return path


def _local_shape(lay: Layout, rank_part: int = 0):
    return lay.local_shape(rank_part)


def _gemm_eff(M, N, K):
    tiles = math.ceil(M / 256) * math.ceil(N / 128)
    waves = math.ceil(tiles / 256)
    quant = tiles / (waves * 256)
    kfac = min(1.0, K / 2048) ** 0.25
    return max(0.05, 0.42 * quant * kfac)


def analytic_cost(layer, cfg: OpConfig, compute_dtype: DataType) -> Tuple[float, float]:
    lo = op_layouts(layer, cfg)
    ins = [l.local_shape(0) for l in lo.inputs]
    outs = [l.local_shape(0) for l in lo.outputs]
    ws = [l.local_shape(0) for l in lo.weights]
    impl = layer.impl
    elem = 2 if compute_dtype == DataType.DT_BF16 else 4
    fl = impl.flops(ins, outs, ws)
    by = impl.mem_bytes(ins, outs, ws, elem)
    if impl.uses_mfma():
        if compute_dtype == DataType.DT_BF16:
            # representative GEMM dims for the tile-quantization term
            out0 = outs[0] if outs else (1,)
            M = max(1, int(math.prod(out0[:-1])))
            N = max(1, int(out0[-1]))
            K = max(1, int(fl / max(1, 2 * M * N)))
            peak = PEAK_BF16 * _gemm_eff(M, N, K)
        else:
            peak = PEAK_FP32 * 0.6
        t = max(fl / peak, by / HBM) + LAUNCH_S * 2
        return t * 1e3, 2.0 * t * 1e3
    t = by / HBM + LAUNCH_S
    return t * 1e3, 2.0 * t * 1e3


def _step_layout(t):
    """A 4-D activation as a training step holds it: channel-last when the kernels take it so
    (kernels.cl_ok: bf16, channels % 8 == 0), so the isolated timing does not pay a layout
    conversion the step never runs (CNN forwards were timed 2-4x slow, r4 calibration)."""
    from .. import kernels as K
    if t.dim() == 4 and K.cl_ok(t, t.shape[1]):
        return t.contiguous(memory_format=torch.channels_last)
    return t


def _saturate(device):
    """Keep the GPU busy while the timed launches are queued, so the events measure device time
    and not Python launch overhead (in a training step the GPU runs behind the host: an op's
    span is its kernels' time; isolated small ops were timed 3-5x too slow, r3/r4 calibration)."""
    try:
        torch.cuda._sleep(2_000_000)
    except Exception:
        pass


def _hot_inputs(layer) -> list:
    """Per input: is it still cache-resident when this op runs in a training step? An input the
    directly preceding op (in the executor's topological order) produced was written microseconds
    before; any other input (a residual stream, a model input, an activation produced several ops
    earlier) comes from HBM. r4 timed every forward input cold, which made MHA +31 % and Linear
    +15 % slow against the step; all-warm had made LayerNorm (whose residual input is cold) fast."""
    m = getattr(layer, "model", None)
    layers = getattr(m, "layers", None) or []
    pos = {id(L): i for i, L in enumerate(layers)}
    me = pos.get(id(layer))
    out = []
    for t in layer.inputs:
        p = getattr(t, "owner_layer", None)
        ok = me is not None and p is not None and p.op_type != OperatorType.OP_INPUT and pos.get(id(p)) == me - 1
        out.append(bool(ok))
    return out


def cost_params_key(layer) -> tuple:
    """The op attributes that can change its cost, as stable strings: initializers are left out
    (they run once, not per step) and object addresses are stripped — the r6 measured-cost table
    missed 25 of BERT-Large's N = 8 entries in a fresh process because repr() of an initializer
    object carries its address."""
    import re
    out = []
    for k, v in layer.impl.params_key():
        if k.endswith("_init") or k.endswith("initializer"):
            continue
        out.append((k, re.sub(r" at 0x[0-9a-fA-F]+", "", v)))
    return tuple(out)


def cost_key(layer, cfg: OpConfig, compute_dtype: DataType) -> tuple:
    """What a measured cost depends on: op, cost-relevant attributes, shard shapes of inputs and
    weights, degrees, dtype, whether the input gradient is needed, the inputs' cache temperature
    and the op's role in a cross-op backward fusion (also the on-disk table's key, as repr)."""
    lo = op_layouts(layer, cfg)
    need_dx0 = bool(layer.inputs) and layer.inputs[0].owner_layer is not None and \
        layer.inputs[0].owner_layer.op_type != OperatorType.OP_INPUT
    # an attention layer's key lengths are timed as a dense batch (fabricate_int_input), so they
    # are left out of the key: the layer shares the measured entry of the same layer without them.
    # Rotary position ids are timed as arange(S), what the layer without them rotates by, and are left
    # out likewise (the rope_* attributes are in cost_params_key, so the rotation itself is priced)
    n_in = 3 if layer.op_type == OperatorType.OP_MULTIHEAD_ATTENTION else len(lo.inputs)
    return (layer.op_type, cost_params_key(layer), tuple(l.local_shape(0) for l in lo.inputs[:n_in]),
            tuple(l.local_shape(0) for l in lo.weights), cfg.degrees, compute_dtype, need_dx0,
            tuple(_hot_inputs(layer)[:n_in]), (dact_fusion_partner(layer) or (None,))[0])


def is_score_bias_input(layer, i: int) -> bool:
    """Input i of `layer` is an attention score bias (the last input of an attention layer built with
    attn_bias): measured as zeros (random values would do, -inf would time an emptier attention) and
    never given a gradient."""
    return layer.op_type in (OperatorType.OP_MULTIHEAD_ATTENTION, OperatorType.OP_SDPA) and \
        bool(layer.attrs.get("attn_bias")) and i == len(layer.inputs) - 1


def is_rope_ids_input(layer, i: int) -> bool:
    """Input i of `layer` is the rotary position ids (attribute rope_positions): the last input of a
    rotary_embedding, the one in front of the score bias (or the last) of an attention layer."""
    if not layer.attrs.get("rope_positions"):
        return False
    if layer.op_type == OperatorType.OP_ROPE:
        return i == 1
    return layer.op_type == OperatorType.OP_MULTIHEAD_ATTENTION and \
        i == len(layer.inputs) - 1 - (1 if layer.attrs.get("attn_bias") else 0)


def fabricate_int_input(layer, i: int, shp, cfg: OpConfig, device) -> torch.Tensor:
    """A stand-in for integer input i of `layer` when its cost is measured: embedding indices over
    the local table, an attention layer's key lengths all equal to Sk (a dense batch: random small
    lengths would time a nearly empty attention), rotary position ids arange(S) in every row (what an
    unpacked batch feeds; they sit behind the key lengths / segment ids, so they are looked for first),
    otherwise 0 / 1."""
    if is_rope_ids_input(layer, i):
        return torch.arange(int(shp[-1]), device=device, dtype=torch.int32).expand(tuple(shp)).contiguous()
    if layer.op_type in (OperatorType.OP_MULTIHEAD_ATTENTION, OperatorType.OP_SDPA) and i == 3 and \
            layer.attrs.get("segment_ids"):  # packed rows: one full-length segment per row
        # (a sliding window needs nothing here: its bounds do not depend on data, window_left / window_right
        # are in cost_params_key, and the layer is timed with its real window, inside that one run)
        return torch.zeros(tuple(shp), device=device, dtype=torch.int32)
    if layer.op_type == OperatorType.OP_MULTIHEAD_ATTENTION and i == 3:
        return torch.full(tuple(shp), int(layer.inputs[1].dims[1]), device=device, dtype=torch.int32)
    if layer.op_type == OperatorType.OP_SDPA and i == 3:
        return torch.full(tuple(shp), int(layer.inputs[1].dims[2]), device=device, dtype=torch.int32)
    hi = 2
    if layer.op_type == OperatorType.OP_EMBEDDING:
        hi = layer.attrs["num_entries"] // max(1, cfg.degrees[-1])
    return torch.randint(0, max(1, hi), tuple(shp), device=device, dtype=torch.int32)


def measure_cost(layer, cfg: OpConfig, compute_dtype: DataType, device, reps: int = 8) -> Tuple[float, float]:
    """Time the op's own forward/backward on this GPU with the shard shapes of `cfg`, the way a
    training step runs it (reference simulator.cu measure_operator_cost; model.cu:38-75):
      * `reps` forwards on distinct input copies, each saving into its own context, then the
        `reps` backwards: a backward reads activations saved long before (cold caches), not the
        ones its own forward just wrote;
      * the input gradient only when the input has a producer (the executor's need_dx0);
      * launches queued behind a device-side busy wait (_saturate)."""
    from ..ops import OpCtx
    lo = op_layouts(layer, cfg)
    need_dx0 = bool(layer.inputs) and layer.inputs[0].owner_layer is not None and \
        layer.inputs[0].owner_layer.op_type != OperatorType.OP_INPUT
    key = cost_key(layer, cfg, compute_dtype)
    if key in _measured:
        return _measured[key]
    hit = _disk_get(key, device)
    if hit is not None:
        _measured[key] = hit
        STATS["table_hits"] += 1
        return hit
    STATS["timed"] += 1
    t_start = time.perf_counter()
    ct = torch.bfloat16 if compute_dtype == DataType.DT_BF16 else torch.float32

    hot = _hot_inputs(layer)
    shared: dict = {}

    def make_inputs():
        xs = []
        for i, (t, l) in enumerate(zip(layer.inputs, lo.inputs)):
            shp = l.local_shape(0)
            if hot[i] and i in shared:  # produced just before this op in a step: one cache-warm copy
                xs.append(shared[i])
                continue
            if t.data_type in (DataType.DT_INT32, DataType.DT_INT64):
                xs.append(fabricate_int_input(layer, i, shp, cfg, device))
            elif is_score_bias_input(layer, i):
                xs.append(torch.zeros(shp, device=device, dtype=torch.float32))
            else:
                xs.append(_step_layout(torch.randn(shp, device=device, dtype=ct)))
            if hot[i]:
                shared[i] = xs[-1]
        # identical tensors in the graph stay identical (fused self-attention)
        seen = {}
        for i, t in enumerate(layer.inputs):
            if t.guid in seen and lo.inputs[i].key() == lo.inputs[seen[t.guid]].key():
                xs[i] = xs[seen[t.guid]]
            else:
                seen.setdefault(t.guid, i)
        return xs

    ws = [torch.randn(l.local_shape(0), device=device, dtype=ct) * 0.02 for l in lo.weights]
    wgrads = [torch.zeros(w.shape, device=device, dtype=torch.float32) for w in ws]
    impl = layer.impl

    fused_relu = relu_fused_into_producer(layer)
    # the executor's backward fusions, as the step runs them
    ln_fused = ln_bias_fusion_producer(layer)
    ln_db = torch.zeros(layer.inputs[0].dims[-1], device=device, dtype=torch.float32) if ln_fused is not None else None
    bias_fused = bias_grad_fused_away(layer)
    # backward act' fusion across two Linears (executor._plan_dact_fusion): the producer's backward
    # skips its act' pass and bias gradient; the consumer's dgrad applies them (kernels.gemm_dact)
    dact = dact_fusion_partner(layer)
    dact_src = None
    if dact is not None and dact[0] == "consumer":
        from ..ops import OpCtx as _Ctx
        P = dact[1]
        rows = math.prod(lo.inputs[0].local_shape(0)[:-1])
        kin = lo.inputs[0].local_shape(0)[-1]
        pctx = _Ctx(layer=P, part_coords=(0,) * len(cfg.degrees), degrees=cfg.degrees, compute_dtype=compute_dtype)
        pctx.saved.update(z=torch.randn(rows, kin, device=device, dtype=ct), has_b=len(P.weights) > 1,
                          z_is_grad=False)
        pctx.wgrads = [torch.zeros(1, device=device), torch.zeros(kin, device=device, dtype=torch.float32)]
        dact_src = (pctx, P.impl.act)

    def make_ctx():
        ctx = OpCtx(layer=layer, part_coords=(0,) * len(cfg.degrees), degrees=cfg.degrees,
                    compute_dtype=compute_dtype)
        ctx.wgrads = wgrads
        ctx.extra["need_dx0"] = need_dx0
        if fused_relu:
            ctx.extra["fused_into_producer"] = True
        if ln_fused is not None:
            ctx.extra["colsum_out"] = ln_db
        if bias_fused:
            ctx.extra["bias_grad_fused"] = True
        if dact is not None and dact[0] == "producer":
            ctx.extra["dact_fused"] = True
        if dact_src is not None:
            ctx.extra["dact_src"] = dact_src
        return ctx

    try:
        # warm-up (kernel selection / tuning happens here, outside the timing)
        c0, x0 = make_ctx(), make_inputs()
        outs = impl.forward(c0, x0, ws)
        douts = [_step_layout(torch.randn(o.shape, device=o.device, dtype=o.dtype)) if o.is_floating_point()
                 else None for o in outs]
        impl.backward(c0, douts)
        del c0, x0, outs
        in_bytes = sum(math.prod(l.local_shape(0)) for l in lo.inputs) * (2 if ct == torch.bfloat16 else 4)
        n = max(2, min(reps, int(math.ceil(768e6 / max(in_bytes, 1)))))  # copies past the 256 MB MALL
        xs_all = [make_inputs() for _ in range(n)]
        ctxs = [make_ctx() for _ in range(n)]
        # weights are cold in a step too (last touched by the previous step's update): one copy per
        # repetition unless that would pass ~1 GiB (Embedding read a warm 62 MB table 22 % fast, r4)
        wbytes = sum(w.numel() * w.element_size() for w in ws)
        ws_all = [ws] + [[w.clone() for w in ws] for _ in range(n - 1)] if wbytes * n <= (1 << 30) else [ws] * n
        torch.cuda.synchronize()
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # device time (queue saturated) and host time (the op's own dispatch): an eager step runs
        # an op no faster than the host issues it, so the cost is the larger of the two.
        # FF_COST_REPS passes (default 3), each term the median over them: one pass let clock and
        # host jitter move a small op's price by tens of percent between searches (r5).
        samples = {"df": [], "hf": [], "db": [], "hb": []}
        for _ in range(max(1, int(os.environ.get("FF_COST_REPS", "3")))):
            # forward on n distinct input copies, each saving into its own context: in a step the
            # inputs of most ops were written long enough before to be out of the caches (timing
            # the forward on one cache-warm input made LayerNorm 16 % and Embedding 17 % fast, r4)
            _saturate(device)
            st.record()
            h0 = time.perf_counter()
            for c, xs, wk in zip(ctxs, xs_all, ws_all):
                impl.forward(c, xs, wk)
            samples["hf"].append((time.perf_counter() - h0) * 1e3 / n)
            en.record()
            en.synchronize()
            samples["df"].append(st.elapsed_time(en) / n)
            # the backward on those n contexts: the activations they saved are cold too
            _saturate(device)
            st.record()
            h0 = time.perf_counter()
            for c in ctxs:
                impl.backward(c, douts)
            samples["hb"].append((time.perf_counter() - h0) * 1e3 / n)
            en.record()
            en.synchronize()
            samples["db"].append(st.elapsed_time(en) / n)
        med = {k: sorted(v)[len(v) // 2] for k, v in samples.items()}
        tf = max(med["df"], med["hf"])
        tb = max(med["db"], med["hb"])
        _disk_put(key, device, tf, tb)
        STATS["timed_s"] += time.perf_counter() - t_start
        del ctxs, xs_all, ws_all
    except Exception:
        tf, tb = analytic_cost(layer, cfg, compute_dtype)
    _measured[key] = (tf, tb)
    return tf, tb


def mem_bytes(layer, cfg: OpConfig, compute_dtype: DataType, training: bool = True) -> float:
    lo = op_layouts(layer, cfg)
    elem = 2 if compute_dtype == DataType.DT_BF16 else 4
    act = sum(math.prod(l.local_shape(0)) for l in lo.outputs) * elem
    act += sum(math.prod(l.local_shape(0)) for l in lo.inputs) * elem if training else 0
    w = sum(math.prod(l.local_shape(0)) for l in lo.weights)
    # fp32 master + fp32 grad + bf16 copy + Adam m, v
    wbytes = w * (4 + 4 + (2 if compute_dtype == DataType.DT_BF16 else 0) + 8) if training else w * elem
    return float(act + wbytes)


def _loss_fused_softmax(layer) -> bool:
    """The model's output softmax under a cross-entropy loss: the executor runs it as ONE fused
    softmax-cross-entropy pass over the logits inside the loss (ops/softmax.py emits the logits
    unchanged), so its standalone softmax forward/backward never runs."""
    from ..type import LossType
    m = getattr(layer, "model", None)
    if m is None or layer.op_type != OperatorType.OP_SOFTMAX:
        return False
    if getattr(m, "loss_type", None) not in (LossType.LOSS_CATEGORICAL_CROSSENTROPY,
                                             LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY):
        return False
    out = m.output_tensor()
    n = len(layer.outputs[0].dims)
    return out is not None and out.guid == layer.outputs[0].guid and layer.attrs.get("dim", -1) % n == n - 1


def fused_xent_cost(layer, cfg: OpConfig, compute_dtype: DataType, measure: bool, device=None):
    """Cost of the fused softmax-cross-entropy pass on this config's shard (forward + backward in
    one kernel: read the logits, write their gradient), charged to the forward."""
    lo = op_layouts(layer, cfg)
    shp = lo.inputs[0].local_shape(0)
    V = shp[-1]
    rows = int(math.prod(shp[:-1]))
    if measure and device is not None and device.type == "cuda" and compute_dtype == DataType.DT_BF16:
        key = ("xent", rows, V)
        if key not in _measured:
            from .. import kernels as K
            x = torch.randn(rows, V, device=device, dtype=torch.bfloat16)
            lab = torch.randint(0, V, (rows,), device=device, dtype=torch.int32)
            lab64 = lab.long()
            macc = torch.zeros(8, device=device, dtype=torch.float32)

            def loss_pass():  # what executor.compute_loss_grad launches around the fused kernel
                acc = torch.zeros(3, dtype=torch.float32, device=device)
                g, _ = K.softmax_xent(x, lab64.reshape(-1).to(torch.int32), 1.0, acc)
                macc[0] += acc[1]
                return g

            loss_pass()
            torch.cuda.synchronize()
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            _saturate(device)
            st.record()
            h0 = time.perf_counter()
            for _ in range(5):
                loss_pass()
            hf = (time.perf_counter() - h0) * 1e3 / 5
            en.record()
            en.synchronize()
            _measured[key] = (max(st.elapsed_time(en) / 5, hf), 0.0)
        return _measured[key]
    elem = 2 if compute_dtype == DataType.DT_BF16 else 4
    t = 2.0 * rows * V * elem / HBM + LAUNCH_S
    return t * 1e3, 0.0


def relu_fused_into_producer(layer) -> bool:
    """The executor applies a ReLU inside the element-wise binary op that produces its input
    (runtime/executor._plan_inplace + _plan_binary_relu: ResNet's residual add + ReLU) when that
    input has no other reader and the producer's backward does not need it: the ReLU's forward is
    then free (its backward still runs). Same conditions, decided from the graph alone."""
    if layer.op_type != OperatorType.OP_RELU or len(layer.inputs) != 1 or os.environ.get("FF_NO_BINARY_RELU") == "1":
        return False
    from ..ops.elementwise import BINARY
    t = layer.inputs[0]
    P = t.owner_layer
    m = getattr(layer, "model", None)
    if P is None or P.op_type not in BINARY or m is None or len(P.outputs) != 1:
        return False
    if P.impl.saves_output() or t.data_type != layer.outputs[0].data_type:
        return False
    out = m.output_tensor()
    if out is not None and out.guid == t.guid:
        return False
    readers = sum(1 for L in m.layers for x in L.inputs if x.guid == t.guid)
    return readers == 1


# Per-op, per-phase floor of an eagerly executed step: the host-side dispatch of one op (Python op
# call, transfers' bookkeeping, kernel launch) when its kernels are shorter than that, measured as
# the in-step span of ops that do no GPU work (flatten, the fused ReLU, a residual add's backward:
# 4.7-6 us; profiles/sim_calibration_*_r4.txt). FF_SIM_OP_FLOOR_US overrides (e.g. ~1 for a
# step replayed from a hipGraph).
OP_FLOOR_MS = float(os.environ.get("FF_SIM_OP_FLOOR_US", "5.0")) * 1e-3


def _sole_reader(t, m):
    return sum(1 for L in m.layers for x in L.inputs if x.guid == t.guid) == 1


def ln_bias_fusion_producer(layer):
    """The producer whose bias gradient a LayerNorm's backward sums for it (executor
    _plan_bias_grad_fusion: a Linear without activation, or an attention's out-projection, whose
    output only this LayerNorm reads), or None."""
    m = getattr(layer, "model", None)
    if layer.op_type != OperatorType.OP_LAYERNORM or m is None or os.environ.get("FF_NO_BIAS_FUSION") == "1":
        return None
    out = m.output_tensor()
    for t in layer.inputs:
        P = t.owner_layer
        if P is None or not _sole_reader(t, m) or (out is not None and out.guid == t.guid):
            continue
        if P.op_type == OperatorType.OP_LINEAR and P.impl.act == 10 and len(P.weights) > 1:
            return P
        if P.op_type == OperatorType.OP_MULTIHEAD_ATTENTION and P.attrs.get("bias", True):
            return P
    return None


def dact_fusion_partner(layer):
    """The executor's backward act' fusion (_plan_dact_fusion), decided from the graph alone:
    ("consumer", P) when this Linear's dgrad applies its producing Linear P's act' (and sums P's
    bias gradient), ("producer", C) when this Linear's act' / bias gradient are done by its sole
    consumer C's dgrad, else None. r5 priced BERT's FFN1 backward with its own bias_act_bwd pass
    (+31 %) and FFN2's without it — errors that cancelled per class but steered per-op choices."""
    m = getattr(layer, "model", None)
    if m is None or layer.op_type != OperatorType.OP_LINEAR or os.environ.get("FF_NO_DACT_FUSION") == "1":
        return None
    out = m.output_tensor()

    def fusable(P, C):
        if P is None or C is None or P.op_type != OperatorType.OP_LINEAR or C.op_type != OperatorType.OP_LINEAR:
            return False
        if getattr(P.impl, "act", 10) == 10 or not C.inputs or C.inputs[0].owner_layer is not P:
            return False
        t = C.inputs[0]
        return _sole_reader(t, m) and not (out is not None and out.guid == t.guid)
    P = layer.inputs[0].owner_layer if layer.inputs else None
    if fusable(P, layer):
        return ("consumer", P)
    for L in m.layers:
        if L.inputs and L.inputs[0].owner_layer is layer and fusable(layer, L):
            return ("producer", L)
    return None


def bias_grad_fused_away(layer) -> bool:
    """The op's own bias-gradient pass is done by the LayerNorm that consumes its output."""
    m = getattr(layer, "model", None)
    if m is None or layer.op_type not in (OperatorType.OP_LINEAR, OperatorType.OP_MULTIHEAD_ATTENTION):
        return False
    o = layer.outputs[0]
    for L in m.layers:
        if L.op_type == OperatorType.OP_LAYERNORM and any(x.guid == o.guid for x in L.inputs):
            return ln_bias_fusion_producer(L) is layer
    return False


def op_cost(layer, cfg: OpConfig, compute_dtype: DataType, measure: bool, device=None):
    if layer.op_type == OperatorType.OP_INPUT:
        return 0.0, 0.0
    on_gpu = measure and device is not None and device.type == "cuda"
    if relu_fused_into_producer(layer):
        f, b = (measure_cost(layer, cfg, compute_dtype, device) if on_gpu else analytic_cost(layer, cfg, compute_dtype))
        f = 0.0
    elif _loss_fused_softmax(layer):
        f, b = fused_xent_cost(layer, cfg, compute_dtype, measure, device)
    elif on_gpu:
        f, b = measure_cost(layer, cfg, compute_dtype, device)
    else:
        f, b = analytic_cost(layer, cfg, compute_dtype)
    return max(f, OP_FLOOR_MS), max(b, OP_FLOOR_MS)
