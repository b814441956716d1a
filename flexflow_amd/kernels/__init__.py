"""Device-dispatching functional layer over the HIP kernel library.

Every function takes torch tensors. On a HIP device the hand-written gfx950 kernels in
`flexflow_amd._C` run (and a missing/unbuilt extension is a hard error, never a silent fallback);
on CPU (unit tests, the `gloo` multi-process tests) an fp32 PyTorch reference of the same math
runs instead. bf16 GEMMs with a fused epilogue (bias + activation + pre-activation store) run on our
MFMA kernels; plain GEMMs are autotuned per call site between our kernels and the vendor library
(hipBLASLt via torch), see gemm().
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

_C = None
_C_err = None


def ext():
    """The compiled HIP extension; raises loudly if it is not built."""
    global _C, _C_err
    if _C is None:
        try:
            from flexflow_amd import _C as mod  # noqa: WPS433
            _C = mod
        except Exception as e:  # pragma: no cover - exercised on GPU boxes only
            _C_err = e
            raise RuntimeError(
                "flexflow_amd._C (HIP kernels) is not built/loadable; run `python build_ext.py` "
                f"(original error: {e})") from e
    return _C


def native(t: torch.Tensor) -> bool:
    return t.is_cuda


def native_device(device) -> bool:
    """native() of a tensor on `device`."""
    return torch.device(device).type == "cuda"


ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_GELU = 10, 11, 12, 13, 14
# kernel-internal: the 'pre-activation' operand holds act'(z) already (stored by the producer's
# forward, linear_fwd(store_grad=True)); the backward multiplies by it
ACT_GRADMUL = 15
ACT_STORE_GRAD = 0x100  # bias_act_fwd flag: write act'(z) into zout instead of z


def act_ref(x, act):
    if act == ACT_RELU:
        return torch.relu(x)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    if act == ACT_TANH:
        return torch.tanh(x)
    if act == ACT_GELU:
        return F.gelu(x)
    return x


def act_grad_ref(z, act):
    if act == ACT_GRADMUL:
        return z
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)
    if act == ACT_SIGMOID:
        s = torch.sigmoid(z)
        return s * (1 - s)
    if act == ACT_TANH:
        t = torch.tanh(z)
        return 1 - t * t
    if act == ACT_GELU:
        cdf = 0.5 * (1 + torch.erf(z * 0.7071067811865476))
        return cdf + z * 0.3989422804014327 * torch.exp(-0.5 * z * z)
    return torch.ones_like(z)


# ----------------------------------------------------------------------------------- GEMM
import os as _os

_TUNE = _os.environ.get("FF_GEMM_TUNE", "1") != "0"
# our kernels: 256-row ping-pong (csrc/kernels/gemm256.hip), 256x128 LDS-DMA (gemm_big.hip), 128x128
IMPLS = {"pp": 6, "k256": 2, "big": 1, "128": 0}
IMPL_DEFAULT = _os.environ.get("FF_GEMM_IMPL", "k256")
_tuned: dict = {}
TUNE_LOG: list = []

# Persistent autotune cache (FF_TUNE_CACHE=<file.json>): the GEMM and convolution choices of a run
# are written at exit (rank 0, atomic rename, merged with what the file held) and read back by the
# next run, whose first step then skips the timing. Only named choices persist; the direct
# hipBLASLt plans ("lt" tuples) hold process-local handles and are re-timed.
_TUNE_CACHE = _os.environ.get("FF_TUNE_CACHE", "")
_cached: dict = {"gemm": {}, "conv": {}}
# call sites whose choice came from a timing (or from the cache): only these are persisted. A choice
# made without timing (FF_GEMM_TUNE=0, first call inside graph capture) is a default, and saving
# it would stop every later run from timing that call site.
_timed: set = set()


def tune_cache_stamp() -> dict:
    """What a cache file is valid for: the device and the kernel build. A file written on another
    GPU model or by another build of _C.so is ignored (its timings do not transfer)."""
    dev = "cpu"
    if torch.cuda.is_available():
        pr = torch.cuda.get_device_properties(0)
        dev = f"{pr.name}|{getattr(pr, 'gcnArchName', '')}|{pr.multi_processor_count}"
    so = _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "flexflow_amd", "_C.so")
    build = "none"
    if _os.path.exists(so):
        import hashlib
        h = hashlib.sha1()
        with open(so, "rb") as f:
            h.update(f.read())
        build = h.hexdigest()[:16]
    return {"device": dev, "build": build}


def _ckey(key) -> str:
    return repr(tuple(str(k) if isinstance(k, torch.dtype) else k for k in key))


def tune_cache_load(path: str) -> int:
    """Read a tune cache file; returns the number of choices loaded (0 if the file is absent)."""
    import json
    if not path or not _os.path.exists(path):
        return 0
    with open(path) as f:
        d = json.load(f)
    stamp = d.get("stamp")
    if stamp is not None and stamp != tune_cache_stamp():
        return 0  # another device or kernel build: re-time everything
    n = 0
    for kind in ("gemm", "conv"):
        for k, v in d.get(kind, {}).items():
            if isinstance(v, str):
                _cached[kind][k] = v
                n += 1
    return n


def tune_cache_save(path: str) -> int:
    """Write the named choices tuned so far (plus those already cached) to `path`."""
    import json
    out = {"gemm": dict(_cached["gemm"]), "conv": dict(_cached["conv"]), "stamp": tune_cache_stamp()}
    for k, v in _tuned.items():
        if isinstance(v, str) and k in _timed:
            out["gemm"][_ckey(k)] = v
    for k, v in _conv_tuned.items():
        if isinstance(v, str):
            out["conv"][_ckey(k)] = v
    tmp = f"{path}.tmp{_os.getpid()}"
    with open(tmp, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    _os.replace(tmp, path)
    return len(out["gemm"]) + len(out["conv"])


def _tune_cache_lookup(kind, key):
    if not _TUNE_CACHE:
        return None
    c = _cached[kind].get(_ckey(key))
    # a cache written by an older build may name a kernel that no longer exists (round 5 removed
    # the 4-wave GEMMs w4 / w4p / w4q): re-tune that site instead of failing at dispatch
    if kind == "gemm" and isinstance(c, str) and not (
            c in IMPLS or c in ("lib", "lib_act", "lib_bias_act", "fused", "fused_pp", "unfused")
            or c.startswith(("pp_sk", "lib_sk"))):
        return None
    return c


if _TUNE_CACHE:
    import atexit as _atexit
    tune_cache_load(_TUNE_CACHE)
    if _os.environ.get("RANK", "0") == "0":
        _atexit.register(lambda: (_tuned or _conv_tuned) and tune_cache_save(_TUNE_CACHE))


def _views(A, B, C, M, N, K, a_k, b_k, lda, ldb, ldc, batch, sA, sB, sC):
    Af = A.as_strided((batch, M, K), (sA, lda, 1)) if a_k else A.as_strided((batch, K, M), (sA, lda, 1)).transpose(1, 2)
    Bf = B.as_strided((batch, N, K), (sB, ldb, 1)).transpose(1, 2) if b_k else B.as_strided((batch, K, N), (sB, ldb, 1))
    Cv = C.as_strided((batch, M, N), (sC, ldc, 1))
    return Af, Bf, Cv


_ADDMM_F32_OUT = [True]  # torch.addmm(out_dtype=fp32, out=C) usable in place

# Library-GEMM solution table. The vendor GEMMs (plain, no fused epilogue) go through PyTorch's
# TunableOp, which picks per (layout, M, N, K) among every hipBLASLt and rocBLAS solution instead of
# the library heuristic; the picks for our models' shapes were measured on an MI355X and ship in
# tuning/tunableop_gfx950.csv (its Validator lines pin the torch / HIP / hipBLASLt / rocBLAS versions,
# a mismatching table is ignored). FF_TUNABLEOP=use (default) reads the table with tuning off
# (unlisted shapes keep the library default), =tune tunes every shape met and writes the table
# to FF_TUNABLEOP_FILE at exit, =off leaves TunableOp alone.
TUNABLE_CSV = _os.environ.get("FF_TUNABLEOP_TABLE") or _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "..",
                                                                     "tuning", "tunableop_gfx950.csv")
_tunable_state = [None]


def tunable_setup():
    if _tunable_state[0] is not None:
        return _tunable_state[0]
    mode = _os.environ.get("FF_TUNABLEOP", "use")
    state = "off"
    if mode != "off" and torch.cuda.is_available():
        import torch.cuda.tunable as tun
        if mode == "tune":
            # tunes every shape it meets from scratch: the file written at exit holds only what
            # this process tuned, so a table read in first would be dropped from it
            tun.enable(True)
            tun.tuning_enable(True)
            tun.set_filename(_os.environ.get("FF_TUNABLEOP_FILE", "tunableop_results.csv"), False)
            state = "tune"
        elif _os.path.exists(TUNABLE_CSV):
            tun.enable(True)
            tun.tuning_enable(False)
            state = "use" if tun.read_file(TUNABLE_CSV) else "rejected"
            if state == "rejected":
                tun.enable(False)
    _tunable_state[0] = state
    return state


def _lib_gemm(A, B, C, M, N, K, a_k, b_k, lda, ldb, ldc, alpha, beta, bias, batch, sA, sB, sC):
    """Plain GEMM on the vendor library (hipBLASLt via torch): bf16 in, bf16 or fp32 out, optional
    bias, beta-accumulate. Only offered for calls without a fused activation epilogue."""
    Af, Bf, Cv = _views(A, B, C, M, N, K, a_k, b_k, lda, ldb, ldc, batch, sA, sB, sC)
    if batch == 1 and alpha == 1.0 and beta == 0.0 and Cv[0].is_contiguous():
        a2, b2, c2 = Af[0], Bf[0], Cv[0]
        if C.dtype == torch.float32:  # bf16 x bf16 -> fp32 straight into C (weight-gradient arena)
            torch.mm(a2, b2, out_dtype=torch.float32, out=c2)
        elif bias is not None:
            torch.addmm(bias.to(a2.dtype), a2, b2, out=c2)
        else:
            torch.mm(a2, b2, out=c2)
        return
    if batch == 1 and alpha == 1.0 and beta == 1.0 and bias is None and Cv[0].is_contiguous():
        a2, b2, c2 = Af[0], Bf[0], Cv[0]
        if C.dtype == a2.dtype:  # C += A.B in the library epilogue (no separate add kernel)
            c2.addmm_(a2, b2)
            return
        if C.dtype == torch.float32 and _ADDMM_F32_OUT[0]:
            try:
                torch.addmm(c2, a2, b2, out_dtype=torch.float32, out=c2)
                return
            except (RuntimeError, TypeError):
                _ADDMM_F32_OUT[0] = False
    if batch == 1:
        a2, b2 = Af[0], Bf[0]
        if C.dtype == torch.float32:
            r = torch.mm(a2, b2, out_dtype=torch.float32)
        elif bias is not None:
            r = torch.addmm(bias.to(a2.dtype), a2, b2)
            bias = None
        else:
            r = torch.mm(a2, b2)
        r = r.unsqueeze(0)
    else:
        r = torch.bmm(Af, Bf)
    if alpha != 1.0:
        r = r * alpha
    if bias is not None:
        r = r + bias.to(r.dtype)
    if beta != 0.0:
        Cv.add_(r.to(Cv.dtype)) if beta == 1.0 else Cv.mul_(beta).add_(r.to(Cv.dtype))
    else:
        Cv.copy_(r)


def _lib_gemm_act(A, B, C, Z, M, N, K, a_k, b_k, lda, ldb, bias, act):
    """Plain library GEMM into the pre-activation buffer, then one fused pass of ours
    (z += bias; C = act(z)): for shapes where the vendor GEMM plus one elementwise pass beats our
    fused epilogue (and torch's bias GEMM, which is slower than its plain one)."""
    zbuf = Z if Z is not None else C
    _lib_gemm(A, B, zbuf, M, N, K, a_k, b_k, lda, ldb, N, 1.0, 0.0, None, 1, 0, 0, 0)
    ext().bias_act_fwd(zbuf, bias, zbuf if bias is not None else None, C, M, N, act)


def _lib_gemm_bias_act(A, B, C, Z, M, N, K, a_k, b_k, lda, ldb, bias, act):
    """Library GEMM with the bias in its epilogue (z = x.w^T + b written once), then our activation
    pass reads z and writes y only: one [M, N] write less than _lib_gemm_act."""
    zbuf = Z if Z is not None else C
    _lib_gemm(A, B, zbuf, M, N, K, a_k, b_k, lda, ldb, N, 1.0, 0.0, bias, 1, 0, 0, 0)
    ext().bias_act_fwd(zbuf, None, None, C, M, N, act)


def _lib_gemm_splitk(A, B, C, M, N, K, a_k, b_k, lda, ldb, beta, S):
    """fp32-output GEMM (a weight gradient: K = tokens, small M x N) as S K-slices of ONE
    strided-batched library GEMM into fp32 slabs, summed (+ beta * C) by our slab_sum kernel. The
    single-shot library GEMM leaves most CUs idle on these shapes (<= 256 output tiles, K >= 8k);
    the batch dimension multiplies its tiles by S."""
    Af, Bf, _ = _views(A, B, C, M, N, K, a_k, b_k, lda, ldb, N, 1, 0, 0, 0)
    a2, b2 = Af[0], Bf[0]
    kc = K // S
    a3 = a2.as_strided((S, M, kc), (kc * a2.stride(1), a2.stride(0), a2.stride(1)))
    b3 = b2.as_strided((S, kc, N), (kc * b2.stride(0), b2.stride(0), b2.stride(1)))
    slabs = torch.empty((S, M, N), device=C.device, dtype=torch.float32)
    if _fold_slabs_ok(C, None, None, ACT_NONE, 1, N, N, M, beta):
        _fold(lambda: torch.bmm(a3, b3, out_dtype=torch.float32, out=slabs),
              lambda: ext().slab_sum(slabs, C, S, beta), (slabs,))
        return
    torch.bmm(a3, b3, out_dtype=torch.float32, out=slabs)
    ext().slab_sum(slabs, C, S, beta)


def _fold_slabs_ok(C, bias, Z, act, batch, ldc, N, M, beta) -> bool:
    """A split-K weight gradient's slab fold may leave the compute stream when the GEMM owns its
    fp32 output (beta = 0: the weight's only user, nothing on the compute stream reads or adds to
    it before the optimizer) and the fold is the plain slab_sum."""
    return (_RED["stream"] is not None and beta == 0.0 and C.dtype == torch.float32 and bias is None and Z is None
            and act == ACT_NONE and batch == 1 and ldc == N and C.is_contiguous() and (M * N) % 4 == 0
            and not torch.cuda.is_current_stream_capturing())


# ------------------------------------------------------------------ hipBLASLt, called directly
# torch.mm reaches hipBLASLt through its heuristic (or TunableOp's table). csrc/kernels/blaslt.cpp
# calls the library directly: it enumerates every solution the library accepts for a call site
# (bias in the epilogue), and gemm() times them once next to our kernels, keeping the fastest.
# Measured on MI355X (profiles/lt_probe_r2.txt): in isolation the best solution beat torch.mm by
# 10-15 % on FFN shapes, but inside the BERT-Large step the TunableOp table already picks as well
# (same-box A/B 50.36/50.58 ms without vs 50.49/50.75 ms with, profiles/lt_ab_r2.txt), and the
# GELU-with-aux and dGELU epilogues that would remove our activation passes have no bf16
# solution on gfx950 in this library build. Kept opt-in (FF_LT=1) for other shapes and models.
LT_WS_BYTES = 64 << 20
EPI_NONE, EPI_BIAS = 0, 1
_LT = _os.environ.get("FF_LT", "0") == "1"  # opt-in: no in-step gain measured (profiles/lt_ab_r2.txt)
_lt_ok = [None]


def _lt_ws(dev):
    from ..runtime.device import DeviceContext
    return DeviceContext.get(dev).workspace("hipblaslt", LT_WS_BYTES, torch.uint8)


def _lt_plan(A, B, C, M, N, K, a_k, b_k, lda, ldb, ldc, batch, sA, sB, sC, bias, beta, epi, max_algos=512):
    X = ext()
    pid, n = X.lt_plan(M, N, K, lda, ldb, ldc, batch, sA, sB, sC, a_k, b_k, C.dtype == torch.float32,
                       bias is not None and bias.dtype == torch.float32, beta != 0.0, epi, ldc, max_algos, True,
                       LT_WS_BYTES, bias, None)
    return pid, n


def _lt_run(pid, algo, A, B, C, bias, alpha, beta):
    st = ext().lt_run(pid, algo, A, B, C, bias, None, float(alpha), float(beta), _lt_ws(C.device))
    if st != 0:
        raise RuntimeError(f"hipBLASLt matmul failed (status {st})")


def _lt_tune(pid, n, A, B, C, bias, alpha, beta):
    """Best (algo, ms) among the plan's candidates: one quick pass, the 6 fastest re-timed."""
    X = ext()
    ws = _lt_ws(C.device)
    quick = []
    for a in range(n):
        if X.lt_run(pid, a, A, B, C, bias, None, float(alpha), float(beta), ws) != 0:
            continue
        quick.append((_time(lambda a=a: X.lt_run(pid, a, A, B, C, bias, None, float(alpha), float(beta), ws), 3), a))
    if not quick:
        return None, float("inf")
    quick.sort()
    fine = [(_time(lambda a=a: X.lt_run(pid, a, A, B, C, bias, None, float(alpha), float(beta), ws), 10), a)
            for _, a in quick[:6]]
    t, a = min(fine)
    return a, t


def _lt_candidates(A, B, C, scratch, M, N, K, a_k, b_k, lda, ldb, ldc, alpha, beta, bias, Z, act, batch, sA, sB,
                   sC, plain, times):
    """Adds hipBLASLt candidates to an autotune table: the GEMM as called (bias in the epilogue), the
    split-K strided-batched form for weight gradients, and GEMM+bias then our activation pass for
    activation epilogues (the library has no GELU-with-aux epilogue for bf16 on gfx950)."""
    try:
        if plain:
            pid, n = _lt_plan(A, B, scratch, M, N, K, a_k, b_k, lda, ldb, ldc, batch, sA, sB, sC, bias, beta,
                              EPI_BIAS if bias is not None else EPI_NONE)
            a, t = _lt_tune(pid, n, A, B, scratch, bias, alpha, beta)
            if a is not None:
                times[("lt", pid, a)] = t
            if C.dtype == torch.float32 and batch == 1 and alpha == 1.0 and bias is None and ldc == N and \
                    (M * N) % 4 == 0 and M * N <= (1 << 25) and K >= 8192:
                for S in ((2, 4, 8) if M * N <= (1 << 24) else (2,)):
                    if K % (S * 8):
                        continue
                    kc = K // S
                    slabs = torch.empty((S, M, N), device=C.device, dtype=torch.float32)
                    pid, n = _lt_plan(A, B, slabs, M, N, kc, a_k, b_k, lda, ldb, N, S, kc if a_k else kc * lda,
                                      kc if b_k else kc * ldb, M * N, None, 0.0, EPI_NONE)
                    a, _ = _lt_tune(pid, n, A, B, slabs, None, 1.0, 0.0)
                    if a is not None:
                        times[("lt_sk", pid, a, S)] = _time(lambda: _lt_splitk(pid, a, A, B, scratch, M, N, S, beta))
        elif (act != ACT_NONE or bias is not None) and alpha == 1.0 and beta == 0.0 and batch == 1 and ldc == N and \
                N % 8 == 0 and C.dtype == torch.bfloat16 and (Z is None or Z.dtype == torch.bfloat16):
            zs = torch.empty_like(C) if Z is not None else scratch
            pid, n = _lt_plan(A, B, zs, M, N, K, a_k, b_k, lda, ldb, ldc, 1, 0, 0, 0, bias, 0.0,
                              EPI_BIAS if bias is not None else EPI_NONE)
            a, _ = _lt_tune(pid, n, A, B, zs, bias, 1.0, 0.0)
            if a is not None:
                times[("lt_act", pid, a)] = _time(lambda: _lt_act(pid, a, A, B, scratch, Z is not None and zs, M, N,
                                                                  bias, act))
    except RuntimeError as e:  # a library refusal is a missing candidate, never a failed step
        TUNE_LOG.append({"M": M, "N": N, "K": K, "lt_error": str(e)})


def _lt_splitk(pid, a, A, B, C, M, N, S, beta):
    slabs = torch.empty((S, M, N), device=C.device, dtype=torch.float32)
    _lt_run(pid, a, A, B, slabs, None, 1.0, 0.0)
    ext().slab_sum(slabs, C, S, beta)


def _lt_act(pid, a, A, B, C, Z, M, N, bias, act):
    zbuf = Z if Z is not None and Z is not False else C
    _lt_run(pid, a, A, B, zbuf, bias, 1.0, 0.0)
    ext().bias_act_fwd(zbuf, None, None, C, M, N, act)


def _lt_dispatch(choice, A, B, C, Z, M, N, K, a_k, b_k, lda, ldb, alpha, beta, bias, act):
    kind = choice[0]
    if kind == "lt":
        _lt_run(choice[1], choice[2], A, B, C, bias, alpha, beta)
    elif kind == "lt_sk":
        _lt_splitk(choice[1], choice[2], A, B, C, M, N, choice[3], beta)
    else:  # "lt_act"
        _lt_act(choice[1], choice[2], A, B, C, Z, M, N, bias, act)


def _time(fn, reps=8):
    fn()
    fn()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(reps):
        fn()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) / reps


_TUNE_ROUNDS = int(_os.environ.get("FF_TUNE_ROUNDS", "3"))
_GEMM_TRACE = _os.environ.get("FF_GEMM_TRACE", "0") == "1"  # print each call site's choice once
_traced = set()
_TUNE_LIB_MARGIN = float(_os.environ.get("FF_TUNE_LIB_MARGIN", "0.03"))


def _time_all(cands, rounds=None):
    """{name: ms} over candidates timed in interleaved rounds (FF_TUNE_ROUNDS, default 3), keeping
    each one's best round: a single pass let clock / neighbour noise pick a slower kernel."""
    times = {}
    for _ in range(rounds or _TUNE_ROUNDS):
        for k, f in cands.items():
            t = _time(f)
            times[k] = min(times.get(k, t), t)
    return times


def gemm(A, B, C, M, N, K, a_k, b_k, lda, ldb, ldc, alpha=1.0, beta=0.0, bias=None, Z=None, act=ACT_NONE,
         batch=1, sA=0, sB=0, sC=0, splitk=None):
    """C = act(alpha*op(A).op(B) + beta*C + bias); raw strided views (see csrc/kernels/gemm.hip).

    On the device, each call site (shape, layouts, epilogue) is autotuned once, outside graph
    capture, among our MFMA kernels (IMPLS) and — for plain GEMMs without a fused activation /
    pre-activation store — the vendor library GEMM. splitk=None lets each kernel pick its split."""
    if native(C) and A.dtype == torch.bfloat16:
        X = ext()
        if _tunable_state[0] is None:
            tunable_setup()

        def ours(impl, out=C, sk=None):
            s = sk if sk is not None else (splitk if splitk is not None else
                                           (X.gemm_pick_splitk(M, N, K, batch, impl) if batch == 1 else 1))
            ws = None
            if s > 1:
                ws = torch.empty(M * N * batch * s, device=C.device, dtype=torch.float32)
                if _fold_slabs_ok(out, bias, Z, act, batch, ldc, N, M, beta):
                    _fold(lambda: X.gemm(A, B, out, bias, Z, M, N, K, lda, ldb, ldc, sA, sB, sC, batch, a_k, b_k,
                                         alpha, beta, act, s, ws, impl, True),
                          lambda: X.slab_sum(ws, out, s, beta), (ws,))
                    return
            X.gemm(A, B, out, bias, Z, M, N, K, lda, ldb, ldc, sA, sB, sC, batch, a_k, b_k, alpha, beta, act,
                   s, ws, impl)

        key = (M, N, K, a_k, b_k, lda, ldb, ldc, batch, C.dtype, bias is not None, Z is not None, act,
               beta != 0.0, splitk)
        choice = _tuned.get(key)
        if choice is None:
            choice = _tune_cache_lookup("gemm", key)
            if choice is not None:
                _tuned[key] = choice
                _timed.add(key)
        if choice is None:
            plain = act == ACT_NONE and Z is None and sC in (0, M * N) and ldc == N
            if not _TUNE or torch.cuda.is_current_stream_capturing():
                choice = IMPL_DEFAULT
            else:
                scratch = torch.zeros_like(C)
                cands = {k: (lambda i=i: ours(i, scratch)) for k, i in IMPLS.items()}
                if C.dtype == torch.float32 and batch == 1 and K >= 8192 and splitk is None:
                    # weight gradients: the ping-pong kernel's split-K factor is tuned like the
                    # library's (fp32 slabs folded by slab_sum); uneven K slices, so any S that fills
                    # the CUs (48 tiles x 5)
                    for S in (2, 3, 4, 5, 6, 8, 16):
                        if K % 64 == 0 and K // 64 >= S:
                            cands[f"pp_sk{S}"] = (lambda S=S: ours(IMPLS["pp"], scratch, S))
                if plain:
                    cands["lib"] = lambda: _lib_gemm(A, B, scratch, M, N, K, a_k, b_k, lda, ldb, ldc, alpha, beta,
                                                     bias, batch, sA, sB, sC)
                    if C.dtype == torch.float32 and batch == 1 and alpha == 1.0 and bias is None and \
                            C.is_contiguous() and (M * N) % 4 == 0 and M * N <= (1 << 25) and K >= 8192:
                        for S in ((2, 4, 8) if M * N <= (1 << 24) else (2,)):
                            if K % (S * 8) == 0:
                                cands[f"lib_sk{S}"] = (lambda S=S: _lib_gemm_splitk(A, B, scratch, M, N, K, a_k, b_k,
                                                                                    lda, ldb, beta, S))
                if (act != ACT_NONE or bias is not None) and alpha == 1.0 and beta == 0.0 and batch == 1 and \
                        ldc == N and N % 8 == 0 and C.dtype == torch.bfloat16 and \
                        (Z is None or Z.dtype == torch.bfloat16):
                    zs = torch.empty_like(C) if Z is not None else None
                    cands["lib_act"] = lambda: _lib_gemm_act(A, B, scratch, zs, M, N, K, a_k, b_k, lda, ldb, bias,
                                                             act)
                    if bias is not None and act != ACT_NONE:
                        cands["lib_bias_act"] = lambda: _lib_gemm_bias_act(A, B, scratch, zs, M, N, K, a_k, b_k, lda,
                                                                           ldb, bias, act)
                red, _RED["stream"] = _RED["stream"], None  # time every candidate with its folds inline
                fq, _FOLDQ["on"] = _FOLDQ["on"], False
                try:
                    times = _time_all(cands)
                finally:
                    _RED["stream"] = red
                    _FOLDQ["on"] = fq
                if _LT and C.dtype in (torch.bfloat16, torch.float32):
                    _lt_candidates(A, B, C, scratch, M, N, K, a_k, b_k, lda, ldb, ldc, alpha, beta, bias, Z, act,
                                   batch, sA, sB, sC, plain, times)
                choice = min(times, key=lambda k: times[k])
                # a library form within FF_TUNE_LIB_MARGIN (default 3 %) of our fastest kernel wins
                # the site: the isolated loop runs on hot caches and an idle chip, and inside the
                # step our persistent kernels (one 512-thread workgroup holding a whole CU) lost
                # such near-ties — the 16384 x 4096 x 1024 NN dgrad picked pp at 0.1307 vs 0.1332
                # and ran 142 us per call in the step (r6 profile)
                lib_keys = [k for k in times if (isinstance(k, str) and k.startswith("lib")) or isinstance(k, tuple)]
                if lib_keys and not (isinstance(choice, str) and choice.startswith("lib")) and \
                        not isinstance(choice, tuple):
                    lb = min(lib_keys, key=lambda k: times[k])
                    if times[lb] <= times[choice] * (1.0 + _TUNE_LIB_MARGIN):
                        choice = lb
                TUNE_LOG.append({"M": M, "N": N, "K": K, "a_k": a_k, "b_k": b_k, "batch": batch, "act": act,
                                 "times_ms": {str(k): round(v, 4) for k, v in times.items()}, "choice": str(choice)})
                _timed.add(key)
            _tuned[key] = choice
        if _GEMM_TRACE and (key, choice) not in _traced:
            _traced.add((key, choice))
            print(f"[gemm] M={M} N={N} K={K} a_k={a_k} b_k={b_k} bias={bias is not None} Z={Z is not None} "
                  f"act={act} beta={beta} -> {choice}", flush=True)
            if _os.environ.get("FF_GEMM_TRACE_STACK"):
                import traceback
                traceback.print_stack(limit=8)
        if isinstance(choice, tuple):
            _lt_dispatch(choice, A, B, C, Z, M, N, K, a_k, b_k, lda, ldb, alpha, beta, bias, act)
        elif isinstance(choice, str) and choice.startswith("pp_sk"):
            ours(IMPLS["pp"], sk=int(choice[5:]))
        elif isinstance(choice, str) and choice.startswith("lib_sk"):
            _lib_gemm_splitk(A, B, C, M, N, K, a_k, b_k, lda, ldb, beta, int(choice[6:]))
        elif choice == "lib":
            _lib_gemm(A, B, C, M, N, K, a_k, b_k, lda, ldb, ldc, alpha, beta, bias, batch, sA, sB, sC)
        elif choice == "lib_act":
            _lib_gemm_act(A, B, C, Z, M, N, K, a_k, b_k, lda, ldb, bias, act)
        elif choice == "lib_bias_act":
            _lib_gemm_bias_act(A, B, C, Z, M, N, K, a_k, b_k, lda, ldb, bias, act)
        else:
            ours(IMPLS[choice])
        return C
    if native(C) and A.dtype == torch.float32 and B.dtype == torch.float32:
        # --dtype fp32 on the device: our f32-input MFMA kernel (csrc/kernels/gemm_f32.hip)
        out = C if C.dtype == torch.float32 else torch.empty(C.shape, device=C.device, dtype=torch.float32)
        if out is not C and beta != 0.0:
            out.copy_(C)
        Zf = Z if (Z is None or Z.dtype == torch.float32) else torch.empty(Z.shape, device=Z.device,
                                                                           dtype=torch.float32)
        ext().gemm_f32(A, B, out, bias, Zf, M, N, K, lda, ldb, ldc, sA, sB, sC, batch, a_k, b_k, alpha, beta, act)
        if out is not C:
            C.copy_(out)
        if Zf is not Z:
            Z.copy_(Zf)
        return C
    # CPU reference (plain torch)
    Af, Bf, Cv = _views(A, B, C, M, N, K, a_k, b_k, lda, ldb, ldc, batch, sA, sB, sC)
    cdt = torch.float32
    r = torch.matmul(Af.to(cdt), Bf.to(cdt)) * alpha
    if beta != 0.0:
        r = r + beta * Cv.to(cdt)
    if bias is not None:
        r = r + bias.to(cdt)
    if Z is not None:
        Z.as_strided((batch, M, N), (sC, ldc, 1)).copy_(r)
    Cv.copy_(act_ref(r, act))
    return C


def gemm_dact(A, B, C, Zp, db, M, N, K, a_k, b_k, lda, ldb, ldc, act):
    """C = (op(A).op(B)) * act'(Zp); db (fp32, optional) += colsum(C): the dgrad GEMM of a Linear
    fused with the activation backward of the Linear that produced its input (BERT: FFN2's dgrad
    and FFN1's GELU'). Autotuned per call site between the fused 256-row MFMA kernel
    (csrc/kernels/gemm256.hip dact epilogue) and the plain GEMM followed by an in-place
    bias_act_bwd pass (what the two ops run unfused)."""
    if native(C) and C.dtype == torch.float32:  # fp32 on the device: our GEMM, then the act' pass
        gemm(A, B, C, M, N, K, a_k, b_k, lda, ldb, ldc)
        ext().bias_act_bwd(C, Zp, C, db, M, N, act)
        return C
    if not native(C) or C.dtype != torch.bfloat16:
        r = A.float() @ B.float().t() if b_k else A.float() @ B.float()
        r = r * act_grad_ref(Zp.float(), act)
        C.copy_(r)
        if db is not None:
            db.add_(r.sum(0))
        return C
    X = ext()

    def fused(out=C, dbo=db, impl=2):
        return X.gemm_dact(A, B, out, Zp, dbo, M, N, K, lda, ldb, ldc, a_k, b_k, act, impl)

    def unfused(out=C, dbo=db):
        gemm(A, B, out, M, N, K, a_k, b_k, lda, ldb, ldc)
        if dbo is not None and _FOLDQ["on"] and _RED["stream"] is None:  # bias fold batched like the others
            ws = torch.empty(int(X.bias_act_bwd_ws(M, N)), device=out.device, dtype=torch.float32)
            _staged_fold(lambda st: X.bias_act_bwd(out, Zp, out, dbo, M, N, act, ws, st), (ws, dbo))
        else:
            X.bias_act_bwd(out, Zp, out, dbo, M, N, act)

    key = ("dact", M, N, K, a_k, b_k, lda, ldb, ldc, act, db is not None)
    choice = _tuned.get(key)
    if choice is None:
        choice = _tune_cache_lookup("gemm", key)
        if choice is not None:
            _tuned[key] = choice
            _timed.add(key)
    if choice is None:
        if not _TUNE or torch.cuda.is_current_stream_capturing():
            choice = "fused_pp"
        else:
            scratch = torch.empty_like(C)
            dbs = torch.zeros_like(db) if db is not None else None
            cands = {}
            if fused(scratch, dbs, 6):  # the ping-pong kernel's DACT epilogue (gemm_pp.hip)
                cands["fused_pp"] = lambda: fused(scratch, dbs, 6)
            if fused(scratch, dbs):
                cands["fused"] = lambda: fused(scratch, dbs)
            if not cands:
                choice = "unfused"
            else:
                fq, _FOLDQ["on"] = _FOLDQ["on"], False  # candidates timed with their folds inline
                try:
                    unfused(scratch, dbs)  # tune the plain GEMM's call site outside the timing
                    cands["unfused"] = lambda: unfused(scratch, dbs)
                    times = _time_all(cands)
                finally:
                    _FOLDQ["on"] = fq
                choice = min(times, key=lambda k: times[k])
                TUNE_LOG.append({"op": "gemm_dact", "M": M, "N": N, "K": K, "a_k": a_k, "b_k": b_k, "act": act,
                                 "times_ms": {k: round(v, 4) for k, v in times.items()}, "choice": choice})
                _timed.add(key)
        _tuned[key] = choice
    if choice == "fused_pp" and fused(impl=6):
        return C
    if choice == "fused" and fused():
        return C
    unfused()
    return C


def linear_fwd(x2d, w, bias, act, save_z, store_grad=False):
    """y = act(x.w^T + b) for x2d [M,K], w [N,K]. Returns (y, z_or_None). store_grad: the second
    value is act'(z) instead of z (the backward then uses ACT_GRADMUL): the consumer's dgrad GEMM
    multiplies by it in its epilogue instead of evaluating act' per element."""
    M, K = x2d.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x2d.device, dtype=x2d.dtype)
    z = torch.empty_like(y) if (save_z and act != ACT_NONE) else None
    if store_grad and z is not None and native(x2d) and x2d.dtype == torch.bfloat16 and w.dtype == x2d.dtype \
            and N % 8 == 0:
        # library GEMM (+ bias) into z, then one pass: y = act(z), z <- act'(z) in place
        _lib_gemm(x2d, w, z, M, N, K, True, True, K, K, N, 1.0, 0.0, bias, 1, 0, 0, 0)
        ext().bias_act_fwd(z, None, z, y, M, N, act | ACT_STORE_GRAD)
        return y, z
    if native(x2d) and x2d.dtype in (torch.bfloat16, torch.float32) and w.dtype == x2d.dtype:
        gemm(x2d, w, y, M, N, K, True, True, K, K, N, bias=bias, Z=z, act=act)
        if store_grad and z is not None:
            z.copy_(act_grad_ref(z.float(), act).to(z.dtype))
        return y, z
    r = x2d.float() @ w.float().t()
    if bias is not None:
        r = r + bias.float()
    if z is not None:
        z.copy_(act_grad_ref(r, act) if store_grad else r)
    y.copy_(act_ref(r, act))
    return y, z


# Transposed weight copies (FF_WT_COPY, default on). The input-gradient GEMM dx = dy . W reads the
# [out, in] weight N-contiguous ("NN"); on MI355X that form is 11-16 % slower than the K-contiguous
# "TN" GEMM of the same M / N / K for BERT-Large's dgrad shapes (in-step tuner timings, library:
# 16384 x 1024 x 4096 0.1045 -> 0.0914 ms, x 3072 0.0801 -> 0.0716, vocabulary 0.726 -> 0.608;
# profiles/dgrad_layout_r6.txt). So every training forward of a Linear / attention projection
# whose input gradient is needed refreshes a persistent W^T [in, out] (transpose16 kernel, ~4 B
# moved per weight element, 0.3 ms per BERT-Large step) on the compute stream, and the backward's
# dgrad reads it. Refreshing every forward keeps the copy exact whichever path wrote the weights
# (optimizer, all-gather, set_weights). Measured alternatives (profiles/wt_copy_ab_r6.txt): the
# refresh on a side stream beside the forward GEMMs (+0.4 ms/step: the transposes' workgroups slowed
# the concurrent GEMMs more than they cost serially), the same with the grid capped at 16
# workgroups (+2.5 ms), and weight gradients on a side stream beside the rest of the backward
# (+0.5 ms once its buffer hazards were joined).
_WT = {"on": None, "step": 0, "in_fwd": False}


def wt_copy_enabled() -> bool:
    if _WT["on"] is None:
        _WT["on"] = _os.environ.get("FF_WT_COPY", "1") != "0"
    return _WT["on"]


def weight_t(store: dict, w: torch.Tensor):
    """store's transposed copy of w [out, in] -> wt [in, out], current for this forward, or None
    when w does not qualify (not a contiguous device bf16 matrix with dims % 8 == 0). Inside an
    executor forward that already refreshed every registered copy in one launch (wt_refresh_all) the
    copy is returned as is; otherwise it is refreshed here and registered for the next batch."""
    if not (wt_copy_enabled() and native(w) and w.dtype == torch.bfloat16 and w.dim() == 2 and w.is_contiguous()
            and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0 and w.data_ptr() % 16 == 0
            and w.numel() < (1 << 31)):
        return None
    buf = store.get("wt_buf")
    src = store.get("wt_src")
    same = src is not None and src.data_ptr() == w.data_ptr() and src.shape == w.shape
    if same and buf is not None and _WT["in_fwd"] and store.get("wt_step") == _WT["step"]:
        return buf
    if buf is None or buf.shape != (w.shape[1], w.shape[0]) or buf.device != w.device:
        buf = store["wt_buf"] = torch.empty(w.shape[1], w.shape[0], device=w.device, dtype=w.dtype)
    ext().transpose2d(w, buf)
    store["wt_src"] = w
    store["wt_step"] = _WT["step"]
    return buf


def wt_refresh_all(stores, cache: dict):
    """Refresh the transposed copies of `stores` (the weight_t stores of one executor's ops) in ONE
    launch (transpose16_batch) — called by the executor at the start of a training forward, once
    the optimizer's writes of the weights are ordered before it; weight_t() then hands the copies
    out without a launch per weight (98 launches of 5-6 us each per BERT-Large step). `cache` keeps
    the device descriptor table between calls. Returns the number of copies refreshed."""
    _WT["step"] += 1
    if not wt_copy_enabled():
        return 0
    items = [st for st in stores if st.get("wt_src") is not None and st.get("wt_buf") is not None]
    if not items:
        return 0
    key = tuple((st["wt_src"].data_ptr(), st["wt_buf"].data_ptr(), st["wt_src"].shape[0], st["wt_src"].shape[1])
                for st in items)
    if cache.get("key") != key:
        rows, tile = [], 0
        for sp, dp, r, c in key:
            rows.append([sp, dp, r, c, tile])
            tile += ((r + 63) // 64) * ((c + 63) // 64)
        cache.update(key=key, desc=torch.tensor(rows, dtype=torch.int64).to(items[0]["wt_buf"].device),
                     n=len(rows), tiles=tile)
    ext().transpose2d_batch(cache["desc"], cache["n"], cache["tiles"])
    for st in items:
        st["wt_step"] = _WT["step"]
    return cache["n"]


def wt_forward(active: bool):
    """The executor marks its training forward (weight_t may then trust wt_refresh_all's copies)."""
    _WT["in_fwd"] = bool(active)


def linear_bwd(dy2d, x2d, w, z, act, dw, db, need_dx=True, dw_beta=1.0, dx_out=None, dact=None, on_dx=None,
               wt=None):
    """Backward of linear_fwd. dw/db are fp32 gradient accumulators (+= ; dw_beta=0 overwrites dw
    when the executor knows this op is the weight's only user). dx_out: an existing input gradient
    [M, K] to accumulate into (dgrad GEMM with beta = 1, no separate add). dact = (z, act, db) of
    the Linear that produced x: the returned dx is then already that producer's pre-activation
    gradient (and its bias gradient is summed), see gemm_dact. on_dx(dx) is called between the
    dgrad and the wgrad GEMM (the executor starts dx's collective there). wt: weight_t()'s W^T for
    a TN dgrad. Returns dx (or None)."""
    M, N = dy2d.shape
    K = x2d.shape[1]
    if act != ACT_NONE:
        dz = bias_act_bwd(dy2d, z, act, db)
    else:
        dz = dy2d
        if db is not None:
            bias_grad(dz, db)
    dx = None
    if dact is not None:
        assert need_dx and dx_out is None
        dx = torch.empty(M, K, device=dy2d.device, dtype=dy2d.dtype)
        if wt is not None and wt.shape == (K, N) and dy2d.dtype == torch.bfloat16:
            gemm_dact(dz, wt, dx, dact[0], dact[2], M, K, N, True, True, N, N, K, dact[1])
        else:
            gemm_dact(dz, w, dx, dact[0], dact[2], M, K, N, True, False, N, K, K, dact[1])
        need_dx = False
        if on_dx is not None:
            on_dx(dx)
    if native(dy2d) and dy2d.dtype in (torch.bfloat16, torch.float32) and w.dtype == dy2d.dtype \
            and x2d.dtype == dy2d.dtype:
        if need_dx:
            dx = dx_out if dx_out is not None else torch.empty(M, K, device=dy2d.device, dtype=dy2d.dtype)
            if wt is not None and wt.shape == (K, N) and dy2d.dtype == torch.bfloat16:
                gemm(dz, wt, dx, M, K, N, True, True, N, N, K, beta=1.0 if dx_out is not None else 0.0)
            else:
                gemm(dz, w, dx, M, K, N, True, False, N, K, K, beta=1.0 if dx_out is not None else 0.0)
            if on_dx is not None:
                on_dx(dx)
        if dw is not None:
            gemm(dz, x2d, dw, N, K, M, False, False, N, K, K, beta=dw_beta)
        return dx
    dzf = dz.float()
    if need_dx:
        dxf = dzf @ w.float()
        if dx_out is not None:
            dx_out.copy_((dx_out.float() + dxf).to(dy2d.dtype))
            dx = dx_out
        else:
            dx = dxf.to(dy2d.dtype)
        if on_dx is not None:
            on_dx(dx)
    if dw is not None:
        if dw_beta == 0.0:
            dw.copy_(dzf.t() @ x2d.float())
        else:
            dw.add_(dzf.t() @ x2d.float())
    return dx


# Deferred gradient reductions. The slab folds that finish a parameter gradient (bias / LayerNorm
# column sums, split-K weight-gradient slabs) are needed by the optimizer, not by the rest of the
# backward: while the executor runs an overlapped update it hands its side stream here, and the
# folds queue on it (behind an event of the compute stream, ahead of the bucket updates queued
# there later) instead of between the backward's GEMMs. set_reduce_stream(None) restores inline folds.
_RED = {"stream": None, "deferred": 0}


def set_reduce_stream(stream):
    _RED["stream"] = stream


def reductions_deferred() -> int:
    return _RED["deferred"]


# Batched parameter-gradient folds. With batching on (the executor turns it on for a training
# backward, FF_FOLD_BATCH=1 default), a bias / LayerNorm backward runs its row pass inline and its
# deterministic column folds are queued (native fold recorder) instead of launched; fold_flush()
# launches the queue as a few col_reduce_batch_kernel launches (up to 24 slab / output pairs each),
# right before a gradient bucket is reduced or updated and at the end of the backward. Same
# arithmetic, same order: bitwise equal gradients; the slab workspaces stay referenced until then.
_FOLDQ = {"on": False, "keep": []}


def set_fold_batching(on: bool):
    _FOLDQ["on"] = bool(on)


def fold_flush():
    if _FOLDQ["keep"]:
        ext().fold_flush()
        _FOLDQ["keep"] = []


def _staged_fold(run, keep):
    """run(stage): stage 1 (row pass) inline, stage 2's folds queued; keep: the slab workspace and
    the fold outputs, referenced until the queue is launched."""
    X = ext()
    run(1)
    X.fold_record(True)
    try:
        run(2)
    finally:
        X.fold_record(False)
    _FOLDQ["keep"].append(keep)


def _fold(main, fold, keep=()):
    """main() on the current stream, then fold() inline or on the reduction stream."""
    main()
    st = _RED["stream"]
    if st is None:
        fold()
        return
    ev = torch.cuda.Event()
    ev.record()
    with torch.cuda.stream(st):
        st.wait_event(ev)
        fold()
    for t in keep:  # workspaces read on the side stream stay allocated until it has run
        t.record_stream(st)
    _RED["deferred"] += 1


def bias_grad(dy2d, db):
    if native(dy2d):
        _bias_act_bwd_dev(dy2d, None, None, db, ACT_NONE)
    else:
        db.add_(dy2d.float().sum(0))


def _bias_act_bwd_dev(dy2d, z, dz, db, act):
    X = ext()
    rows, cols = dy2d.shape
    if db is None or _RED["stream"] is None:
        if db is not None and _FOLDQ["on"]:
            ws = torch.empty(int(X.bias_act_bwd_ws(rows, cols)), device=dy2d.device, dtype=torch.float32)
            _staged_fold(lambda st: X.bias_act_bwd(dy2d, z, dz, db, rows, cols, act, ws, st), (ws, db))
            return
        X.bias_act_bwd(dy2d, z, dz, db, rows, cols, act)
        return
    ws = torch.empty(int(X.bias_act_bwd_ws(rows, cols)), device=dy2d.device, dtype=torch.float32)
    _fold(lambda: X.bias_act_bwd(dy2d, z, dz, db, rows, cols, act, ws, 1),
          lambda: X.bias_act_bwd(dy2d, z, dz, db, rows, cols, act, ws, 2), (ws,))


def bias_act_bwd(dy2d, z, act, db):
    """dz = dy*act'(z); db += colsum(dz)."""
    if native(dy2d):
        dz = torch.empty_like(dy2d)
        _bias_act_bwd_dev(dy2d, z, dz, db, act)
        return dz
    dz = (dy2d.float() * act_grad_ref(z.float(), act)).to(dy2d.dtype)
    if db is not None:
        db.add_(dz.float().sum(0))
    return dz


def bmm(a, b, trans_a=False, trans_b=False, out=None):
    """Batched matmul over the leading dims: a [..., M, K] (or [..., K, M] if trans_a)."""
    if native(a) and a.dtype in (torch.bfloat16, torch.float32) and b.dtype == a.dtype and a.is_contiguous() \
            and b.is_contiguous():
        batch = int(math.prod(a.shape[:-2]))
        M = a.shape[-1] if trans_a else a.shape[-2]
        K = a.shape[-2] if trans_a else a.shape[-1]
        N = b.shape[-2] if trans_b else b.shape[-1]
        if out is None:
            out = torch.empty(*a.shape[:-2], M, N, device=a.device, dtype=a.dtype)
        gemm(a, b, out, M, N, K, not trans_a, trans_b, a.shape[-1], b.shape[-1], N, batch=batch,
             sA=a.shape[-1] * a.shape[-2], sB=b.shape[-1] * b.shape[-2], sC=M * N, splitk=1)
        return out
    aa = a.transpose(-1, -2) if trans_a else a
    bb = b.transpose(-1, -2) if trans_b else b
    r = torch.matmul(aa.float(), bb.float()).to(a.dtype)
    if out is not None:
        out.copy_(r)
        return out
    return r


# ------------------------------------------------------------------------------ attention
def attn_supported(x, D):
    return native(x) and x.dtype == torch.bfloat16 and D in (64, 128)


def attn_padded_dim(x, kd, vd):
    """Head dim (64 / 128) the MFMA attention runs a smaller equal q/k/v head dim at, zero-padded;
    0 when the kernels cannot run it (different q/k and v dims, or above 128)."""
    if not (native(x) and x.dtype == torch.bfloat16) or kd != vd or kd > 128:
        return 0
    return 64 if kd <= 64 else 128


def attn_key_lens(key_lens, B, device):
    """The per-sample key lengths of a right-padded batch as the kernels take them: contiguous int32
    [B] ([B, 1] is flattened) on `device`, or None. Values are clamped to [0, Sk] where they are
    read, on the device; nothing here looks at them."""
    if key_lens is None:
        return None
    kl = key_lens.reshape(-1)
    if kl.numel() != B:
        raise ValueError(f"key_lengths: expected {B} entries (one per sample), got {tuple(key_lens.shape)}")
    if kl.dtype != torch.int32 or kl.device != device or not kl.is_contiguous():
        kl = kl.to(device=device, dtype=torch.int32).contiguous()
    return kl


# ---- packed sequences: per-token segment ids
def attn_seg_bounds_ref(ids):
    """lo, hi (int32, ids' shape) of segment ids [B, S], on ids' device with tensor ops only: a segment
    is a maximal run of equal ids >= 0 and [lo[b, i], hi[b, i]) is the run position i lies in; a
    padding position (id < 0) gets the empty run lo = hi = i. What attn_seg_bounds computes on the
    device (attn_seg_bounds_kernel)."""
    B, S = ids.shape
    pos = torch.arange(S, device=ids.device, dtype=torch.int64).expand(B, S)
    start = torch.ones(B, S, dtype=torch.bool, device=ids.device)
    start[:, 1:] = ids[:, 1:] != ids[:, :-1]
    lo = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), 1).values
    end = torch.ones(B, S, dtype=torch.bool, device=ids.device)  # a run ends behind position i
    end[:, :-1] = start[:, 1:]
    nxt = torch.where(end, pos + 1, torch.full_like(pos, S))
    hi = torch.flip(torch.cummin(torch.flip(nxt, (1,)), 1).values, (1,))
    pad = ids < 0
    return torch.where(pad, pos, lo).to(torch.int32), torch.where(pad, pos, hi).to(torch.int32)


def attn_seg_bounds(ids):
    """lo, hi of segment ids (int32 [B, S]): the bounds kernel on a native device (one launch, nothing
    read on the host), attn_seg_bounds_ref elsewhere."""
    if not native(ids):
        return attn_seg_bounds_ref(ids)
    if ids.dim() != 2 or ids.dtype != torch.int32:
        raise ValueError(f"attn_seg_bounds: ids must be int32 [B, S], got {ids.dtype} {list(ids.shape)}")
    ids = ids.contiguous()
    lo, hi = torch.empty_like(ids), torch.empty_like(ids)
    ext().attn_seg_bounds(ids, lo, hi)
    return lo, hi


# ---- sliding-window (local) attention: flash-attention's window_size convention
def attn_window_config(what, window, Sq, Sk, causal):
    """The builders' `window` argument, checked and normalised: None | w | (left, right) -> None or the
    hashable pair (left, right) with -1 for an unbounded side. Query i sees key j iff i - left <= j <=
    i + right (and j <= i with causal). None or -1 is unbounded, an int w is (w, w). A side >= S - 1 is
    unbounded, causal drops the right side, and when nothing bounded remains the result is None: the
    layer is then built as if the keyword had not been given."""
    if window is None:
        return None
    import numbers
    if isinstance(window, numbers.Real):
        sides = (window, window)
    elif isinstance(window, (tuple, list)):
        sides = tuple(window)
    else:
        sides = ()
    if len(sides) != 2:
        raise ValueError(f"{what}: window must be None, an int or (left, right), got {window!r}")
    out = []
    for w in sides:
        w = -1 if w is None else w
        if isinstance(w, bool) or int(w) != w or int(w) < -1:
            raise ValueError(f"{what}: window sizes must be ints >= 0 (None or -1: unbounded), got {window!r}")
        out.append(int(w))
    left, right = out
    if causal:
        right = -1
    if left < 0 and right < 0:
        return None
    if Sq != Sk:
        raise ValueError(f"{what}: window needs Sq == Sk (positions are row indices), got Sq {Sq}, Sk {Sk}")
    left = -1 if left >= Sq - 1 else left
    right = -1 if right >= Sq - 1 else right
    return None if left < 0 and right < 0 else (left, right)


def attn_band_bounds_ref(S, left, right, lo=None, hi=None, B=1, device="cpu"):
    """lo, hi, klo, khi (int32 [B, S]) of the band `left` / `right` (-1: unbounded), optionally inside the
    runs lo / hi of attn_seg_bounds, with tensor ops on any device: query i sees the keys [lo[i], hi[i])
    = [max(seg_lo, i - left), min(seg_hi, i + right + 1)) and key j is seen by the queries [klo[j],
    khi[j]) = [max(seg_lo, j - right), min(seg_hi, j + left + 1)). A padding position (lo == hi) keeps
    its empty interval on both sides. What attn_band_bounds computes on the device."""
    if lo is not None:
        B, device = lo.shape[0], lo.device
        slo, shi = lo.to(torch.int64), hi.to(torch.int64)
    else:
        slo = torch.zeros(B, S, dtype=torch.int64, device=device)
        shi = torch.full((B, S), S, dtype=torch.int64, device=device)
    pos = torch.arange(S, device=device, dtype=torch.int64).expand(B, S)
    pad = slo >= shi

    def side(before, behind):
        a = slo if before < 0 else torch.maximum(slo, pos - before)
        b = shi if behind < 0 else torch.minimum(shi, pos + behind + 1)
        return torch.where(pad, slo, a).to(torch.int32), torch.where(pad, shi, b).to(torch.int32)

    return (*side(left, right), *side(right, left))


def attn_band_bounds(S, left, right, lo=None, hi=None, B=1, device="cpu"):
    """attn_band_bounds_ref by one launch of attn_band_bounds_kernel on a native device (nothing read on
    the host), attn_band_bounds_ref elsewhere."""
    if (lo is None) != (hi is None):
        raise ValueError("attn_band_bounds: the run bounds lo and hi come together")
    dev = lo.device if lo is not None else torch.device(device)
    if not native_device(dev):
        return attn_band_bounds_ref(S, left, right, lo, hi, B, device)
    if lo is not None:
        B = lo.shape[0]
        lo, hi = lo.contiguous(), hi.contiguous()
    out = tuple(torch.empty(B, S, dtype=torch.int32, device=dev) for _ in range(4))
    ext().attn_band_bounds(int(left), int(right), lo, hi, *out)
    return out


_BAND_BOUNDS: dict = {}


def attn_band_bounds_const(B, S, left, right, device):
    """The four bound arrays of a window without segment ids, a constant of the layer: built once per
    (device, S, left, right) for at least B rows (every row is the same, so a shard takes the first B of
    them) and cached. The executor builds it when it sets a layer up, outside any captured region. An
    entry is never replaced or freed: a captured graph holds raw pointers into it, so a later caller
    that needs more rows gets a further entry beside the earlier ones."""
    entries = _BAND_BOUNDS.setdefault((str(torch.device(device)), int(S), int(left), int(right)), [])
    t = next((e for e in entries if e[0].shape[0] >= B), None)
    if t is None:
        t = attn_band_bounds(S, left, right, B=B, device=device)
        entries.append(t)
    return tuple(x[:B] for x in t)


def band_mask_ref(S, left, right, causal, ids=None):
    """bool [B|1, S, S] from the definition: query i sees key j iff i - left <= j <= i + right (-1:
    unbounded), j <= i with causal, and, with segment ids [B, S], both lie in one run of equal ids >= 0."""
    dev = ids.device if ids is not None else "cpu"
    i = torch.arange(S, device=dev)[:, None]
    j = torch.arange(S, device=dev)[None, :]
    m = torch.ones(S, S, dtype=torch.bool, device=dev)
    if left >= 0:
        m = m & (j >= i - left)
    if right >= 0:
        m = m & (j <= i + right)
    if causal:
        m = m & (j <= i)
    if ids is None:
        return m[None]
    return m[None] & segment_mask_ref(ids)


class AttnSegments(tuple):
    """(ids, lo, hi, klo, khi, window) as the attention paths take segments and / or a window; the first
    three are what attn_segments returned before a window existed."""
    ids = property(lambda s: s[0])
    window = property(lambda s: s[5])


def attn_segments(segment_ids, B, S, device, window=None):
    """Per-token segment ids of packed rows and / or a sliding window (attn_window_config's pair) as the
    attention paths take them: (ids, lo, hi, klo, khi, window), or None when neither is given. ids is a
    contiguous int32 [B, S] on `device` (None without segment ids); lo / hi are the key interval of
    every query (the run of attn_seg_bounds, cut to the band by attn_band_bounds), klo / khi the query
    interval of every key (None without a window: the relation is then symmetric), all on a native
    device and None elsewhere (the reference path builds its mask from ids and window). Nothing here
    reads a value on the host."""
    if segment_ids is None and window is None:
        return None
    device = torch.device(device)
    on_device = native_device(device)  # one predicate for the run bounds and the band bounds
    ids = lo = hi = klo = khi = None
    if segment_ids is not None:
        ids = segment_ids.reshape(segment_ids.shape[0], -1) if segment_ids.dim() == 3 else segment_ids
        if tuple(ids.shape) != (B, S):
            raise ValueError(f"segment_ids: expected [{B}, {S}] (one id per token), got {list(segment_ids.shape)}")
        if ids.dtype != torch.int32 or ids.device != device or not ids.is_contiguous():
            ids = ids.to(device=device, dtype=torch.int32).contiguous()
        lo, hi = attn_seg_bounds(ids) if on_device else (None, None)
    if window is not None and on_device:
        if ids is None:
            lo, hi, klo, khi = attn_band_bounds_const(B, S, window[0], window[1], device)
        else:
            lo, hi, klo, khi = attn_band_bounds(S, window[0], window[1], lo, hi, B=B, device=device)
    return AttnSegments((ids, lo, hi, klo, khi, window))


def segment_mask_ref(ids, causal=False):
    """bool [B, S, S]: query i sees key j (same run of equal ids >= 0; j <= i with causal)."""
    lo, hi = attn_seg_bounds_ref(ids)
    j = torch.arange(ids.shape[1], device=ids.device)[None, None, :]
    m = (j >= lo[:, :, None]) & (j < hi[:, :, None])
    if causal:
        m = m & (j <= torch.arange(ids.shape[1], device=ids.device)[None, :, None])
    return m


def _seg_kw(segments, key_lens, bias, Sq, Sk):
    """segments (attn_segments) -> the bindings' keyword arguments."""
    if segments is None:
        return {}
    if key_lens is not None or bias is not None:
        raise ValueError("attention: segment_ids / window cannot be combined with key_lengths or attn_bias")
    if segments[1] is None:
        raise ValueError("attention: the segment bounds are missing (attn_segments on a native device)")
    kw = dict(seg_lo=segments[1], seg_hi=segments[2])
    if len(segments) > 3 and segments[3] is not None:  # a window: the key side is the transpose
        kw.update(seg_klo=segments[3], seg_khi=segments[4])
    return kw


# ---- attention dropout: csrc/kernels/attn_dropout.h is the device definition, this is its mirror
_ADROP_GOLD = 0x9E3779B97F4A7C15
_ADROP_STEP = 0xD1B54A32D192ED03
_ADROP_KMUL = 0x9E3779B1


def attn_dropout_thr(p) -> int:
    """8-bit drop threshold round(256 p) of an attention dropout rate p in [0, 1): an element is
    dropped iff its hash byte is below it, so the effective rate is p_eff = thr / 256 (and the
    kept elements are scaled by 256 / (256 - thr)). 0 means no dropout."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"attention dropout rate must be in [0, 1), got {p}")
    return min(int(256.0 * p + 0.5), 255)


def attn_dropout_seed(seed, layer_id) -> int:
    """seed and layer id folded into the 64-bit stream key the kernels take (unsigned)."""
    M = (1 << 64) - 1
    return _mix64((int(seed) * _ADROP_GOLD + int(layer_id)) & M)


def _xshift(z, s):  # logical right shift of a wrapped (signed) int64 tensor
    return (z >> s) & ((1 << (64 - s)) - 1)


def _mix64_t(z):
    z = (z ^ _xshift(z, 30)) * _to_signed(0xBF58476D1CE4E5B9)
    z = (z ^ _xshift(z, 27)) * _to_signed(0x94D049BB133111EB)
    return z ^ _xshift(z, 31)


def attn_dropout_keep_ref(seed, layer_id, step, B, H, Sq, Sk, p, b0=0, h0=0, H_total=None, device="cpu"):
    """The attention dropout keep-mask as bool [B, H, Sq, Sk]: element [b, h, q, k] is that of
    global sample b0 + b and global head h0 + h (of H_total heads; default H) of layer `layer_id`
    in training step `step` (an int, or a one-element int64 tensor that is read on its device only).
    A pure function of (seed, layer_id, step, b, h, q, k), evaluated with wrapped int64 torch ops
    exactly as attn_dropout.h evaluates it on the device."""
    thr = attn_dropout_thr(p)
    H_total = H if H_total is None else int(H_total)
    dev = torch.device(device)
    i64 = dict(dtype=torch.int64, device=dev)
    step_t = step.to(**i64).reshape(()) if isinstance(step, torch.Tensor) else torch.tensor(int(step), **i64)
    s = _mix64_t(step_t * _to_signed(_ADROP_STEP) + _to_signed(attn_dropout_seed(seed, layer_id)))
    bh = ((torch.arange(B, **i64) + int(b0))[:, None] * H_total + (torch.arange(H, **i64) + int(h0))[None, :])
    hk = _mix64_t(s + bh * _to_signed(_ADROP_GOLD))  # [B, H]
    rk = _xshift(_mix64_t(hk[:, :, None] + torch.arange(Sq, **i64) * _to_signed(_ADROP_GOLD)), 32)  # [B, H, Sq]
    m32 = 0xFFFFFFFF
    kq = torch.arange((Sk + 3) // 4, **i64)
    x = (rk[..., None] + kq * _ADROP_KMUL) & m32  # [B, H, Sq, Sk/4]
    x = ((x ^ (x >> 16)) * 0x85EBCA6B) & m32
    x = ((x ^ (x >> 13)) * 0xC2B2AE35) & m32
    x = x ^ (x >> 16)
    byts = (x[..., None] >> (8 * torch.arange(4, **i64))) & 255  # [B, H, Sq, Sk/4, 4]
    return (byts >= thr).reshape(B, H, Sq, -1)[..., :Sk]


def attn_dropout_mask(B, H, Sq, Sk, thr, rng_step, rng_seed, b0=0, h0=0, H_total=None, device=None):
    """The keep-mask as the device function draws it (attn_dropout_mask_kernel): bool [B, H, Sq, Sk]."""
    out = torch.empty(B, H, Sq, Sk, dtype=torch.uint8, device=device if device is not None else rng_step.device)
    ext().attn_dropout_mask(out, B, H, Sq, Sk, b0, h0, H if H_total is None else H_total, thr, rng_step,
                            _to_signed(rng_seed))
    return out.bool()


def _drop_kw(drop):
    """drop: None or (thr, rng_step, rng_seed, b0, h0, H_total) -> the bindings' keyword arguments."""
    if not drop or not drop[0]:
        return {}
    thr, step, seed, b0, h0, H_total = drop
    return dict(drop_thr=int(thr), rng_step=step, rng_seed=_to_signed(int(seed)), b0=int(b0), h0=int(h0),
                H_total=int(H_total))


def attn_score_bias(bias, B, H, Sq, Sk, device):
    """The additive score bias as the kernels take it: fp32 [Bb, Hb, Sq, Sk] with Bb in {1, B} and Hb in
    {1, H}, contiguous, on `device` (cast / copied once here when it is not), or None. Scores are
    scale * q.k + bias; -inf (or anything so negative that bias * log2(e) overflows fp32, such as
    finfo.min) removes the key, a row with no key left gives zero output and zero gradients. The bias
    takes no gradient."""
    if bias is None:
        return None
    if bias.dim() != 4 or bias.shape[0] not in (1, B) or bias.shape[1] not in (1, H) or \
            tuple(bias.shape[2:]) != (Sq, Sk):
        raise ValueError(f"attention score bias: expected [1|{B}, 1|{H}, {Sq}, {Sk}], got {list(bias.shape)}")
    if not bias.is_floating_point():
        raise ValueError(f"attention score bias must be a float tensor, got {bias.dtype}")
    if bias.dtype != torch.float32 or bias.device != device or not bias.is_contiguous():
        bias = bias.to(device=device, dtype=torch.float32).contiguous()
    return bias


def _sbias_kw(bias, B, H, Sq, Sk, device):
    """bias (attn_score_bias) -> the bindings' keyword arguments; a dim of extent 1 broadcasts (stride 0)."""
    bias = attn_score_bias(bias, B, H, Sq, Sk, device)
    if bias is None:
        return {}
    Bb, Hb = bias.shape[:2]
    return dict(sbias=bias, sbias_sb=Hb * Sq * Sk if Bb > 1 else 0, sbias_sh=Sq * Sk if Hb > 1 else 0)


def attn_kv_heads(H, Hkv):
    """The KV head count of grouped-query attention: Hkv (None: H) must divide H; query head h reads KV
    head h // (H // Hkv), torch's enable_gqa / repeat_interleave convention."""
    if Hkv is None:
        return int(H)
    Hkv = int(Hkv)
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"attention: the KV head count ({Hkv}) must divide the head count ({H})")
    return Hkv


def flash_attn_fwd(q, qs, k, ks, v, vs, o, os_, B, H, Sq, Sk, D, scale, causal, key_lens=None, drop=None, bias=None,
                   segments=None, Hkv=None):
    """Hkv: optional KV head count (attn_kv_heads): k / v and their strides ks / vs then hold Hkv heads.
    segments: optional packed-sequence runs and / or a sliding window (attn_segments): attention stays
    inside a token's own run and band, a padding position gives o = 0, lse = +inf. key_lens: optional int32 [B] device tensor; key j of sample b is attended iff j < key_lens[b]
    (a length of 0: o = 0, lse = +inf). drop: optional attention dropout (thr, rng_step, rng_seed, b0,
    h0, H_total), see _drop_kw / attn_dropout_keep_ref; lse is that of the undropped softmax.
    bias: optional score bias [1|B, 1|H, Sq, Sk] (attn_score_bias)."""
    lse = torch.empty(B * H * Sq, device=q.device, dtype=torch.float32)
    ext().attn_fwd(q, qs, k, ks, v, vs, o, os_, lse, B, H, Sq, Sk, D, scale, causal,
                   attn_key_lens(key_lens, B, q.device), **_drop_kw(drop), **_sbias_kw(bias, B, H, Sq, Sk, q.device),
                   **_seg_kw(segments, key_lens, bias, Sq, Sk), Hkv=attn_kv_heads(H, Hkv))
    return lse


def flash_attn_bwd(q, qs, k, ks, v, vs, o, os_, do, dos, lse, dq, dqs, dk, dks, dv, dvs, B, H, Sq, Sk, D, scale,
                   causal, dbias=None, key_lens=None, drop=None, bias=None, segments=None, Hkv=None):
    """Hkv: as in flash_attn_fwd; dk / dv and dks / dvs hold Hkv heads, each the sum over its group of
    query heads (fp32, one rounding, the same bits on every run), and the bias gradient is never fused
    (a dbias given with Hkv < H is left untouched, returns False).
    segments: as in flash_attn_fwd; the dq / dk / dv rows of padding positions are written as zeros,
    and the segment kernels never fuse the bias gradient (returns False).
    key_lens: as in flash_attn_fwd; dk / dv rows at or past a sample's length are written as zeros.
    drop: as in flash_attn_fwd, with the counter value the forward saw; the dropout kernels never fuse
    the bias gradient (returns False). bias: the forward's score bias; it takes no gradient, and the
    score bias kernels never fuse the (QKV projection's) bias gradient either.
    dbias: optional contiguous fp32 [3*H*D] bias gradient of a fused [B,S,3,H,D] QKV projection
    (dq/dk/dv inside one dqkv buffer). Returns True when the kernel added the column sums of dq / dk /
    dv into it (attn_bwd1b_kernel, non-causal); False: the caller still owes that bias gradient."""
    X = ext()
    from ..runtime.device import DeviceContext
    # dQ partial slabs + delta: one arena buffer shared (stream-ordered) by every attention layer
    Hkv = attn_kv_heads(H, Hkv)
    if Hkv < H:
        dbias = None  # laid out for [3][H][D]: the caller sums the projection biases, as with dropout
    ws = DeviceContext.get(q.device).workspace("attn_bwd", X.attn_bwd_ws(B, H, Sq, Sk, D, Hkv))
    return bool(X.attn_bwd(q, qs, k, ks, v, vs, o, os_, do, dos, lse, dq, dqs, dk, dks, dv, dvs, ws, B, H, Sq, Sk, D,
                           scale, causal, dbias, attn_key_lens(key_lens, B, q.device), **_drop_kw(drop),
                           **_sbias_kw(bias, B, H, Sq, Sk, q.device), **_seg_kw(segments, key_lens, bias, Sq, Sk),
                           Hkv=Hkv))


# ------------------------------------------------------------------ rotary position embedding (rope.hip)
_ROPE_TABLES: dict = {}


def rope_config(what, rotary, D, S_max):
    """`rotary` (True or a dict with dim / base / interleaved / scale / inv_freq / max_positions) of head
    rows of width D, checked and normalised into plain hashable values: (dim, base, interleaved, scale,
    inv_freq tuple or None, max_positions). max_positions defaults to S_max (the longest sequence)."""
    cfg = {} if rotary is True else dict(rotary)
    unknown = set(cfg) - {"dim", "base", "interleaved", "scale", "inv_freq", "max_positions"}
    if unknown:
        raise ValueError(f"{what}: unknown rotary keys {sorted(unknown)}")
    rd = int(cfg.get("dim") or D)
    if rd < 2 or rd % 2 or rd > D:
        raise ValueError(f"{what}: the rotary dim must be even and in [2, {D}] (the head dim), got {rd}")
    base, scale = float(cfg.get("base", 10000.0)), float(cfg.get("scale", 1.0))
    if not (base > 0 and math.isfinite(base) and scale > 0 and math.isfinite(scale)):
        raise ValueError(f"{what}: rotary base and scale must be positive and finite, got {base}, {scale}")
    inv = cfg.get("inv_freq")
    if inv is not None:
        inv = tuple(float(f) for f in (inv.tolist() if hasattr(inv, "tolist") else inv))
        if len(inv) != rd // 2:
            raise ValueError(f"{what}: rotary inv_freq must hold dim / 2 = {rd // 2} values, got {len(inv)}")
    maxp = int(cfg.get("max_positions") or S_max)
    if maxp < S_max:
        raise ValueError(f"{what}: rotary max_positions ({maxp}) is below the sequence length ({S_max})")
    return rd, base, bool(cfg.get("interleaved", False)), scale, inv, maxp


def rope_table(rd, max_positions, base=10000.0, scale=1.0, inv_freq=None, device="cpu"):
    """The (cos, sin) table the rotation reads: fp32 [max_positions, rd / 2, 2] on `device`, entry (p, i)
    the cosine and sine of (p / scale) * inv_freq[i] with inv_freq[i] = base^(-2i / rd) (or the explicit
    list), computed on the host in float64 and rounded once. Cached per (device, rd, base, scale,
    inv_freq, max_positions); a cache miss uploads, so call it where an op is set up and not under
    stream capture."""
    device = torch.device(device)
    inv = None if inv_freq is None else tuple(float(f) for f in inv_freq)
    key = (str(device), int(rd), float(base), float(scale), inv, int(max_positions))
    t = _ROPE_TABLES.get(key)
    if t is None:
        if rd < 2 or rd % 2:
            raise ValueError(f"rope_table: rd must be even and >= 2, got {rd}")
        if inv is not None and len(inv) != rd // 2:
            raise ValueError(f"rope_table: inv_freq must hold rd / 2 = {rd // 2} values, got {len(inv)}")
        f = (torch.tensor(inv, dtype=torch.float64) if inv is not None
             else float(base) ** (-torch.arange(0, rd, 2, dtype=torch.float64) / rd))
        ang = (torch.arange(int(max_positions), dtype=torch.float64) / float(scale))[:, None] * f[None, :]
        t = torch.stack((torch.cos(ang), torch.sin(ang)), -1).to(torch.float32).contiguous().to(device)
        _ROPE_TABLES[key] = t
    return t


def rope_ref(x, table, pos=None, rd=None, interleaved=False, inverse=False):
    """Plain-torch rotation of x [B, H, S, D] (any strides) by the definition rope.hip implements: the
    first rd columns of every head row rotate by table[p] with p = pos[b, s] clamped to the table (pos
    None: p = s), pairs (i, i + rd/2) or, interleaved, (2i, 2i + 1); y1 = x1 c - x2 s, y2 = x2 c + x1 s
    in fp32 with one rounding to x's dtype; inverse takes -s. Columns [rd, D) are returned unchanged."""
    B, H, S, D = x.shape
    rd = D if rd is None else int(rd)
    half = rd // 2
    maxp = table.shape[0]
    if pos is None:
        p = torch.arange(S, device=x.device).clamp(max=maxp - 1)[None, :].expand(B, S)
    else:
        p = pos.reshape(B, S).to(device=x.device, dtype=torch.int64).clamp(0, maxp - 1)
    cs = table.to(x.device)[p]  # [B, S, half, 2]
    c, s = cs[..., 0][:, None], cs[..., 1][:, None]
    if inverse:
        s = -s
    xf = x[..., :rd].float()
    x1, x2 = (xf[..., 0::2], xf[..., 1::2]) if interleaved else (xf[..., :half], xf[..., half:])
    y1, y2 = x1 * c - x2 * s, x2 * c + x1 * s
    out = x.clone()
    if interleaved:
        out[..., 0:rd:2], out[..., 1:rd:2] = y1.to(x.dtype), y2.to(x.dtype)
    else:
        out[..., :half], out[..., half:rd] = y1.to(x.dtype), y2.to(x.dtype)
    return out


@torch.no_grad()
def rope(q, qs, k, ks, B, H, Hkv, Sq, Sk, D, rd, table, pos=None, interleaved=False, inverse=False, q_out=None,
         k_out=None):
    """Rotate the head rows of q (and of k unless it is None) by their positions in ONE launch (rope.hip).
    q / k are flat buffers read as [B, H | Hkv, Sq | Sk, D] through (batch, head, row) element strides qs
    / ks with contiguous D, e.g. the Q and K thirds of a fused [T, 3, H, D] buffer. In place unless q_out
    / k_out (buffers addressed by the same strides) are given; out of place, columns [rd, D) are copied.
    table: rope_table(...) on q's device; pos: int32 [B, S] position ids (then Sq == Sk), read and
    clamped to the table on the device, or None for position = row index. inverse: the backward (the
    rotation by the negated angle). Without a native device the same definition runs as rope_ref."""
    q_out = q if q_out is None else q_out
    k_out = k if k_out is None else k_out
    if pos is not None:
        if k is not None and Sq != Sk:
            raise ValueError(f"rope: position ids need Sq == Sk, got {Sq} and {Sk}")
        if tuple(pos.shape) != (B, Sq) or pos.dtype != torch.int32:
            raise ValueError(f"rope: position ids must be int32 [{B}, {Sq}], got {pos.dtype} {list(pos.shape)}")
        if pos.device != q.device or not pos.is_contiguous():
            pos = pos.to(q.device).contiguous()
    elif table.shape[0] < max(Sq, Sk if k is not None else 0):
        raise ValueError(f"rope: the table holds {table.shape[0]} positions, the sequence has {max(Sq, Sk)}")
    if native(q):
        ext().rope(q, q_out, list(qs), H, Sq, k, k_out, list(ks) if k is not None else [0, 0, 0], Hkv, Sk, B, D, rd,
                   table, pos, bool(interleaved), bool(inverse))
        return
    for t, o, st, H_, S_ in ((q, q_out, qs, H, Sq), (k, k_out, ks, Hkv, Sk)):
        if t is None:
            continue
        view = t.as_strided((B, H_, S_, D), (st[0], st[1], st[2], 1))
        y = rope_ref(view, table, pos, rd, interleaved, inverse)
        o.as_strided((B, H_, S_, D), (st[0], st[1], st[2], 1)).copy_(y)


# ---------------------------------------------------------------------------- layer norm
def layernorm_fwd(x2d, res2d, gamma, beta, eps, save_sum):
    """y = LN(x + res). Returns (y, sum_or_x, mean, rstd)."""
    rows, cols = x2d.shape
    if native(x2d):
        y = torch.empty_like(x2d)
        mean = torch.empty(rows, device=x2d.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        s = torch.empty_like(x2d) if res2d is not None else None
        ext().layernorm_fwd(x2d, res2d, s, gamma, beta, y, mean, rstd, rows, cols, eps)
        return y, (s if s is not None else x2d), mean, rstd
    xs = x2d.float() + (res2d.float() if res2d is not None else 0)
    mean = xs.mean(-1)
    var = xs.var(-1, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    y = (xs - mean[:, None]) * rstd[:, None]
    if gamma is not None:
        y = y * gamma.float()
    if beta is not None:
        y = y + beta.float()
    return y.to(x2d.dtype), xs.to(x2d.dtype), mean, rstd


def layernorm_bwd(dy2d, xs2d, gamma, mean, rstd, dgamma, dbeta, dres=None, dsum=None):
    """dx of LayerNorm; dgamma/dbeta += their column sums; dsum (fp32 [cols]) += colsum(dx), the bias
    gradient of the Linear feeding this LayerNorm, computed in the same pass."""
    rows, cols = dy2d.shape
    if native(dy2d):
        X = ext()
        dx = torch.empty_like(dy2d)
        if _RED["stream"] is None or (dgamma is None and dbeta is None and dsum is None):
            if _FOLDQ["on"] and not (dgamma is None and dbeta is None and dsum is None):
                ws = torch.empty(int(X.layernorm_bwd_ws(rows, cols)), device=dy2d.device, dtype=torch.float32)
                _staged_fold(lambda st: X.layernorm_bwd(dy2d, xs2d, gamma, mean, rstd, dx, dres, dgamma, dbeta,
                                                        rows, cols, False, dsum, ws, st),
                             (ws, dgamma, dbeta, dsum))
                return dx
            X.layernorm_bwd(dy2d, xs2d, gamma, mean, rstd, dx, dres, dgamma, dbeta, rows, cols, False, dsum)
            return dx
        ws = torch.empty(int(X.layernorm_bwd_ws(rows, cols)), device=dy2d.device, dtype=torch.float32)
        _fold(lambda: X.layernorm_bwd(dy2d, xs2d, gamma, mean, rstd, dx, dres, dgamma, dbeta, rows, cols, False,
                                      dsum, ws, 1),
              lambda: X.layernorm_bwd(dy2d, xs2d, gamma, mean, rstd, dx, dres, dgamma, dbeta, rows, cols, False,
                                      dsum, ws, 2), (ws, dx))
        return dx
    xh = (xs2d.float() - mean[:, None]) * rstd[:, None]
    dy = dy2d.float()
    g = dy * (gamma.float() if gamma is not None else 1.0)
    s1 = g.mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    dx = rstd[:, None] * (g - s1 - xh * s2)
    if dres is not None:
        dx = dx + dres.float()
    if dgamma is not None:
        dgamma.add_((dy * xh).sum(0))
    if dbeta is not None:
        dbeta.add_(dy.sum(0))
    dxo = dx.to(dy2d.dtype)
    if dsum is not None:
        dsum.add_(dxo.float().sum(0))
    return dxo


# ----------------------------------------------------------------------------- softmax/loss
def softmax_fwd(x2d):
    if native(x2d):
        x2d = x2d.contiguous()  # the kernels index rows flat; empty_like would keep a transpose's strides
        y = torch.empty_like(x2d)
        ext().softmax_fwd(x2d, y, x2d.shape[0], x2d.shape[1], 1.0)
        return y
    return torch.softmax(x2d.float(), -1).to(x2d.dtype)


def softmax_bwd(y2d, dy2d):
    if native(y2d):
        y2d, dy2d = y2d.contiguous(), dy2d.contiguous()
        dx = torch.empty_like(dy2d)
        ext().softmax_bwd(y2d, dy2d, dx, y2d.shape[0], y2d.shape[1], 1.0, False)
        return dx
    y = y2d.float()
    d = dy2d.float()
    return (y * (d - (d * y).sum(-1, keepdim=True))).to(dy2d.dtype)


def count_valid_labels(labels, ignore_index):
    """Number of labels != ignore_index as fp32 [1] on the labels' device (overwritten, no host read):
    the `valid_count` of the loss kernels below."""
    if native(labels):
        return ext().count_valid_labels(labels.reshape(-1).to(torch.int32).contiguous(), int(ignore_index))
    return (labels != int(ignore_index)).sum().float().reshape(1)


def _ignore_kw(ignore_index, valid_count):
    """Trailing arguments of the native loss entry points: none without ignore_index, so a call
    without one is the call it always was."""
    if ignore_index is None:
        if valid_count is not None:
            raise ValueError("valid_count needs ignore_index")
        return {}
    return {"ignore_index": int(ignore_index), "valid_count": valid_count}


def _ignore_scale(gscale, valid_count):
    """CPU fallbacks: the gradient scale, 1 / max(valid_count, 1) when the count is given."""
    return gscale if valid_count is None else 1.0 / valid_count.float().clamp_min(1.0)


def xent_grad(probs2d, labels, onehot, gscale, sparse, ignore_index=None, valid_count=None):
    """(p - y)*gscale and per-row CE; labels int32 [rows] (sparse) or onehot [rows, C].
    ignore_index / valid_count (sparse only): as in softmax_xent."""
    rows, cols = probs2d.shape
    if ignore_index is not None and not sparse:
        raise ValueError("ignore_index needs sparse labels")
    kw = _ignore_kw(ignore_index, valid_count)
    if native(probs2d):
        probs2d = probs2d.contiguous()
        d = torch.empty_like(probs2d)
        loss = torch.empty(rows, device=probs2d.device, dtype=torch.float32)
        ext().xent_grad(probs2d, labels.contiguous() if sparse else None,
                        None if sparse else onehot.contiguous(), d, loss, rows, cols, gscale, sparse, **kw)
        return d, loss
    p = probs2d.float()
    if ignore_index is not None:
        keep = labels.long() != int(ignore_index)
        t = F.one_hot(labels.long().clamp(0, cols - 1), cols).float()
        t = t * ((labels.long() >= 0) & (labels.long() < cols))[:, None]
        # where, not a product: an ignored row may hold NaN, which must not leak
        d = torch.where(keep[:, None], (p - t) * _ignore_scale(gscale, valid_count), torch.zeros_like(p))
        loss = torch.where(keep, -(t * torch.log(p.clamp_min(1e-12))).sum(-1), torch.zeros(rows))
        return d.to(probs2d.dtype), loss
    t = F.one_hot(labels.long(), cols).float() if sparse else onehot.float()
    d = ((p - t) * gscale).to(probs2d.dtype)
    loss = -(t * torch.log(p.clamp_min(1e-12))).sum(-1)
    return d, loss


def softmax_xent(logits2d, labels, gscale, acc3=None, ignore_index=None, valid_count=None):
    """(dlogits, per-row CE) of softmax + sparse CE; acc3 (fp32 [3]) += {correct, sum CE, rows}.
    ignore_index: rows with that label are left out (gradient row +0, CE 0, logits never read, not
    counted in acc3). valid_count (fp32 [1] on the device, count_valid_labels): the gradient scale
    is 1 / max(valid_count, 1) instead of gscale."""
    rows, cols = logits2d.shape
    kw = _ignore_kw(ignore_index, valid_count)
    if native(logits2d):
        logits2d = logits2d.contiguous()
        d = torch.empty_like(logits2d)
        loss = torch.empty(rows, device=logits2d.device, dtype=torch.float32)
        ext().softmax_xent(logits2d, labels.contiguous(), loss, d, rows, cols, gscale, acc3, **kw)
        return d, loss
    lf = logits2d.float()
    p = torch.softmax(lf, -1)
    lab = labels.long()
    valid = (lab >= 0) & (lab < cols)
    t = F.one_hot(lab.clamp(0, cols - 1), cols).float() * valid[:, None]
    ce = -(t * torch.log_softmax(lf, -1)).sum(-1)
    if ignore_index is not None:
        keep = lab != int(ignore_index)
        ce = torch.where(keep, ce, torch.zeros_like(ce))
        if acc3 is not None:
            acc3[0] += ((lf.argmax(-1) == lab) & keep).float().sum()
            acc3[1] += ce.sum()
            acc3[2] += keep.float().sum()
        d = torch.where(keep[:, None], (p - t) * _ignore_scale(gscale, valid_count), torch.zeros_like(p))
        return d.to(logits2d.dtype), ce
    if acc3 is not None:
        acc3[0] += (lf.argmax(-1) == lab).float().sum()
        acc3[1] += ce.sum()
        acc3[2] += rows
    return ((p - t) * gscale).to(logits2d.dtype), ce


def mse_grad(pred, label, gscale):
    if native(pred):
        pred = pred.contiguous()
        d = torch.empty_like(pred)
        loss = torch.zeros(1, device=pred.device, dtype=torch.float32)
        ext().mse_grad(pred, label.to(pred.dtype).contiguous(), d, loss, gscale)
        return d, loss
    diff = pred.float() - label.float()
    return (diff * gscale).to(pred.dtype), (diff * diff).sum().reshape(1)


# ------------------------------------------------------------------------------ elementwise
U = dict(relu=0, sigmoid=1, tanh=2, elu=3, gelu=4, exp=5, sin=6, cos=7, rsqrt=8, pow=9, identity=10,
         scalar_multiply=11, scalar_add=12, scalar_sub=13, scalar_true_divide=14, scalar_floor_divide=15, log=16,
         sqrt=17, neg=18, leaky_relu=19)
# unary functions behind the reference's element-unary set (codes continue ops.h UnaryOp). Do not merge
# this into U: tests/test_small_kernels_gpu.py asserts at import that set(U) equals its own list of cases
# (one per reference op), so a new name in U stops that whole module from being collected
U_MORE = dict(silu=20)


def unary_code(name) -> int:
    c = U.get(name, U_MORE.get(name))
    if c is None:
        raise ValueError(f"unknown unary function {name!r}")
    return c


def unary_ref(name, x, s):
    xf = x.float()
    r = {
        "relu": lambda: torch.relu(xf), "sigmoid": lambda: torch.sigmoid(xf), "tanh": lambda: torch.tanh(xf),
        "elu": lambda: F.elu(xf), "gelu": lambda: F.gelu(xf), "exp": lambda: torch.exp(xf),
        "sin": lambda: torch.sin(xf), "cos": lambda: torch.cos(xf), "rsqrt": lambda: torch.rsqrt(xf),
        "pow": lambda: torch.pow(xf, s), "identity": lambda: xf, "scalar_multiply": lambda: xf * s,
        "scalar_add": lambda: xf + s, "scalar_sub": lambda: xf - s, "scalar_true_divide": lambda: xf / s,
        "scalar_floor_divide": lambda: torch.floor(xf / s), "log": lambda: torch.log(xf),
        "sqrt": lambda: torch.sqrt(xf), "neg": lambda: -xf, "leaky_relu": lambda: F.leaky_relu(xf, s),
        "silu": lambda: F.silu(xf),
    }[name]()
    return r.to(x.dtype)


# ------------------------------------------------------------------ activation layout
# CNN activations live channel-last on the device in bf16 (NCHW logical shape, NHWC memory:
# torch.channels_last): the convolutions' implicit GEMMs read them in place and write their outputs
# channel-last, batch norm / pooling / channel sums have channel-last kernels (csrc/kernels/cnn.hip)
# and the elementwise ops preserve the layout, so no per-op NCHW <-> NHWC copies remain.
# FF_CHANNELS_LAST=0 keeps NCHW everywhere. CPU / fp32 tensors are always NCHW.
CHANNELS_LAST = _os.environ.get("FF_CHANNELS_LAST", "1") != "0"


def is_nhwc(t):
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)


def cl_ok(t, c):
    """May t (per-group channel count c) be processed channel-last?"""
    return CHANNELS_LAST and t.dim() == 4 and t.dtype == torch.bfloat16 and c % 8 == 0 and native(t)


def cl_dense(t, nhwc):
    """t dense in the requested layout (no copy when it already is)."""
    if nhwc:
        return t if is_nhwc(t) else t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()


def act_dense(t):
    """A 4-D activation dense in the layout its kernels take (channel-last when cl_ok)."""
    if t.dim() != 4:
        return t.contiguous()
    return cl_dense(t, cl_ok(t, t.shape[1]))


def _dense(t):
    """t itself when its memory is dense in NCHW or channel-last order, else a dense copy keeping
    a channel-last view (e.g. a channel slice of a channel-last tensor) channel-last."""
    if t.is_contiguous() or is_nhwc(t):
        return t
    if t.dim() == 4 and t.stride(1) == 1:
        return t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()


dense = _dense


def _like(t, ref):
    """t dense in ref's memory order (ref dense, same shape): elementwise kernels index both flat."""
    if ref.is_contiguous():
        return t.contiguous()
    return cl_dense(t, True)


def unary_fwd(name, x, s=0.0, out=None):
    """y = f(x); out=x computes in place (elementwise, same index: safe)."""
    if native(x) and x.dtype in (torch.bfloat16, torch.float32):
        xc = _dense(x)
        y = out if out is not None else torch.empty_like(xc)
        ext().unary_fwd(xc, y, unary_code(name), float(s))
        return y
    r = unary_ref(name, x, s)
    if out is not None:
        out.copy_(r)
        return out
    return r


def unary_bwd(name, x, y, dy, s=0.0):
    if native(x) and x.dtype in (torch.bfloat16, torch.float32):
        xc = _dense(x)
        dyc = _like(dy, xc)
        dx = torch.empty_like(dyc)
        ext().unary_bwd(xc, _like(y, xc), dyc, dx, unary_code(name), float(s), False)
        return dx
    xr = x.detach().float().requires_grad_()
    out = unary_ref(name, xr, s).float() if name != "identity" else xr * 1.0
    (g,) = torch.autograd.grad(out, xr, dy.float())
    return g.to(dy.dtype)


# ------------------------------------------------------------------ gated linear units (glu.hip)
GLU_ACTS = dict(silu=0, gelu=1, gelu_tanh=2, relu=3, sigmoid=4)


def glu_act_code(what, act) -> int:
    if act not in GLU_ACTS:
        raise ValueError(f"{what}: unknown activation {act!r} (one of {sorted(GLU_ACTS)})")
    return GLU_ACTS[act]


def _glu_act_f32(gf, act):
    if act == "silu":
        return gf * torch.sigmoid(gf)
    if act == "gelu":
        return F.gelu(gf)
    if act == "gelu_tanh":
        return F.gelu(gf, approximate="tanh")
    if act == "relu":
        return torch.relu(gf)
    if act == "sigmoid":
        return torch.sigmoid(gf)
    raise ValueError(f"glu: unknown activation {act!r} (one of {sorted(GLU_ACTS)})")


def glu_ref(g, u, act):
    """y = act(g) * u by the definition glu.hip implements: plain torch, fp32 arithmetic, one rounding to
    g's dtype. act: silu (x sigmoid(x)), gelu (erf form), gelu_tanh, relu, sigmoid. The CPU path."""
    return (_glu_act_f32(g.float(), act) * u.float()).to(g.dtype)


def _glu_2d(what, t, like=None):
    """t as a [rows, F] view (no copy) when its leading dims collapse and its last dim is contiguous;
    otherwise a contiguous copy's view."""
    if like is not None and (tuple(t.shape) != tuple(like.shape) or t.dtype != like.dtype):
        raise ValueError(f"{what}: operands must share one shape and dtype, got {list(t.shape)} {t.dtype} and "
                         f"{list(like.shape)} {like.dtype}")
    if t.dim() == 0:
        raise ValueError(f"{what}: operands need at least one dim")
    F_ = t.shape[-1]
    if t.dim() == 2 and (F_ <= 1 or t.stride(1) == 1):
        return t
    if t.dim() == 1:
        return t.unsqueeze(0) if (F_ <= 1 or t.stride(0) == 1) else t.contiguous().unsqueeze(0)
    if F_ <= 1 or t.stride(-1) == 1:
        try:
            return t.view(-1, F_)  # raises where the leading dims do not collapse into one stride
        except RuntimeError:
            pass
    return t.contiguous().view(-1, F_)


def _glu_out(what, out, like):
    if tuple(out.shape) != tuple(like.shape) or out.dtype != like.dtype or out.device != like.device:
        raise ValueError(f"{what}: an output must have the operands' shape, dtype and device, got "
                         f"{list(out.shape)} {out.dtype}")
    o2 = _glu_2d(what, out)
    if o2.data_ptr() != out.data_ptr():  # _glu_2d had to copy
        raise ValueError(f"{what}: an output must be a strided view with a contiguous last dim whose leading dims "
                         f"collapse, got strides {list(out.stride())}")
    return o2


@torch.no_grad()
def glu_fwd(g, u, act, out=None, max_blocks=0):
    """y = act(g) * u in ONE launch (glu.hip). g / u: same shape and dtype, any strided views with a
    contiguous last dim whose leading dims collapse to one row stride (two tensors, the halves x[..., :F]
    / x[..., F:] of a packed buffer, views into wider buffers: none is copied); other layouts are made
    contiguous first. out: a view of the same kind to write into. Without a native device, or for other
    dtypes than bf16 / fp32, the same definition runs as glu_ref."""
    code = glu_act_code("glu_fwd", act)
    g2 = _glu_2d("glu_fwd", g)
    u2 = _glu_2d("glu_fwd", u, g)
    if out is None:
        out = torch.empty(g.shape, dtype=g.dtype, device=g.device)
    o2 = _glu_out("glu_fwd", out, g)
    if native(g) and g.dtype in (torch.bfloat16, torch.float32):
        ext().glu_fwd(g2, u2, o2, code, int(max_blocks))
    else:
        o2.copy_(glu_ref(g2, u2, act))
    return out


def glu_bwd(g, u, dy, act, dg=None, du=None, max_blocks=0):
    """(dg, du) = (dy * u * act'(g), dy * act(g)) in ONE launch; act(g) and act'(g) are recomputed from
    g. dg / du: views to write into (e.g. the halves of one [.., 2F] gradient buffer), as glu_fwd's
    out. Without a native device: autograd through glu_ref's arithmetic."""
    code = glu_act_code("glu_bwd", act)
    g2 = _glu_2d("glu_bwd", g)
    u2 = _glu_2d("glu_bwd", u, g)
    dy2 = _glu_2d("glu_bwd", dy, g)
    if dg is None:
        dg = torch.empty(g.shape, dtype=g.dtype, device=g.device)
    if du is None:
        du = torch.empty(g.shape, dtype=g.dtype, device=g.device)
    dg2, du2 = _glu_out("glu_bwd", dg, g), _glu_out("glu_bwd", du, g)
    if native(g) and g.dtype in (torch.bfloat16, torch.float32):
        with torch.no_grad():
            ext().glu_bwd(g2, u2, dy2, dg2, du2, code, int(max_blocks))
        return dg, du
    gr = g2.detach().float().requires_grad_()
    ur = u2.detach().float().requires_grad_()
    with torch.enable_grad():
        y = _glu_act_f32(gr, act) * ur
    a, b = torch.autograd.grad(y, (gr, ur), dy2.detach().float())
    with torch.no_grad():
        dg2.copy_(a)
        du2.copy_(b)
    return dg, du


B = dict(add=0, sub=1, mul=2, div=3, max=4, min=5)


def _bcast_desc(a, b, out_shape):
    nd = len(out_shape)

    def strides(t):
        shp = [1] * (nd - t.dim()) + list(t.shape)
        st = [0] * (nd - t.dim()) + list(t.stride())
        return [0 if shp[i] == 1 and out_shape[i] != 1 else st[i] for i in range(nd)]

    return list(out_shape), strides(a), strides(b)


def binary_fwd(name, a, b, relu=False):
    """c = a (op) b, optionally followed by ReLU in the same pass (relu=True)."""
    out_shape = torch.broadcast_shapes(a.shape, b.shape)
    if native(a) and a.dtype in (torch.bfloat16, torch.float32) and len(out_shape) <= 6:
        if b.dtype != a.dtype:
            b = b.to(a.dtype)
        same = tuple(a.shape) == tuple(b.shape) == tuple(out_shape)
        if same:  # flat over the common memory order (NCHW or channel-last)
            a = _dense(a)
            b = _like(b, a)
            c = torch.empty_like(a)
        else:
            c = torch.empty(out_shape, device=a.device, dtype=a.dtype)
        shp, sa, sb = _bcast_desc(a, b, out_shape)
        ext().binary_fwd(a, b, c, B[name] | (0x100 if relu else 0), shp, sa, sb, same)
        return c
    af, bf = a.float(), b.float()
    r = {"add": af + bf, "sub": af - bf, "mul": af * bf, "div": af / bf, "max": torch.maximum(af, bf),
         "min": torch.minimum(af, bf)}[name]
    if relu:
        r = torch.relu(r)
    return r.to(a.dtype)


def _reduce_to(g, shape):
    if tuple(g.shape) == tuple(shape):
        return g
    nd = g.dim()
    shp = [1] * (nd - len(shape)) + list(shape)
    dims = [i for i in range(nd) if shp[i] == 1 and g.shape[i] != 1]
    r = g.float().sum(dim=dims, keepdim=True) if dims else g.float()
    return r.reshape(shape).to(g.dtype)


def binary_bwd(name, a, b, dc, need_a=True, need_b=True):
    out_shape = dc.shape
    if native(dc) and dc.dtype in (torch.bfloat16, torch.float32) and len(out_shape) <= 6:
        bb = b.to(a.dtype) if b.dtype != a.dtype else b
        same = tuple(a.shape) == tuple(b.shape) == tuple(out_shape)
        if same:  # flat over dc's memory order
            dc = _dense(dc)
            a, bb = _like(a, dc), _like(bb, dc)
            da = torch.empty_like(dc) if need_a else None
            db = torch.empty_like(dc) if need_b else None
        else:
            dc = dc.contiguous()
            da = torch.empty(out_shape, device=dc.device, dtype=dc.dtype) if need_a else None
            db = torch.empty(out_shape, device=dc.device, dtype=dc.dtype) if need_b else None
        shp, sa, sb = _bcast_desc(a, bb, out_shape)
        ext().binary_bwd(a, bb, dc, da, db, B[name], shp, sa, sb, same)
        return (_reduce_to(da, a.shape) if need_a else None), (_reduce_to(db, b.shape) if need_b else None)
    ar = a.detach().float().requires_grad_()
    br = b.detach().float().requires_grad_()
    out = {"add": lambda: ar + br, "sub": lambda: ar - br, "mul": lambda: ar * br, "div": lambda: ar / br,
           "max": lambda: torch.maximum(ar, br), "min": lambda: torch.minimum(ar, br)}[name]()
    ga, gb = torch.autograd.grad(out, (ar, br), dc.float())
    return (ga.to(a.dtype) if need_a else None), (gb.to(b.dtype) if need_b else None)


def dropout_fwd(x, rate, seed, offset):
    if native(x) and x.dtype in (torch.bfloat16, torch.float32):
        xc = x.contiguous()
        y = torch.empty_like(xc)
        mask = torch.empty(xc.numel(), device=x.device, dtype=torch.uint8)
        ext().dropout_fwd(xc, y, mask, float(rate), int(seed), int(offset))
        return y, mask
    g = torch.Generator().manual_seed(int(seed) * 1000003 + int(offset))
    keep = (torch.rand(x.shape, generator=g) >= rate).to(x.device)
    return (x * keep / (1 - rate)).to(x.dtype), keep.to(torch.uint8).view(-1)


def dropout_bwd(dy, mask, rate):
    if native(dy):
        dy = dy.contiguous()  # the mask is in row-major order (dropout_fwd)
        dx = torch.empty_like(dy)
        ext().dropout_bwd(dy, mask, dx, float(rate), False)
        return dx
    return (dy * mask.view(dy.shape).to(dy.dtype) / (1 - rate)).to(dy.dtype)


# ----------------------------------------------------------------------------- embedding
def embedding_fwd(idx, table, bag, avg):
    dim = table.shape[-1]
    n = idx.numel() // bag
    if native(table) and table.dtype in (torch.bfloat16, torch.float32):
        out = torch.empty(n, dim, device=table.device, dtype=table.dtype)
        ii = idx.contiguous()
        if ii.dtype not in (torch.int32, torch.int64):
            ii = ii.to(torch.int64)
        ext().embedding_fwd(ii, table.contiguous(), out, n, bag, dim, avg)
        return out
    ii = idx.long().reshape(n, bag)
    valid = (ii >= 0) & (ii < table.shape[0])  # ids owned by another vocab shard contribute 0
    rows = table.float()[ii.clamp(0, table.shape[0] - 1)] * valid[..., None]
    r = rows.sum(1) / bag if avg else rows.sum(1)
    return r.to(table.dtype)


def embedding_bwd(idx, dout2d, dtable, bag, avg):
    dim = dtable.shape[-1]
    n = idx.numel() // bag
    if native(dout2d):
        ii = idx.contiguous()
        if ii.dtype not in (torch.int32, torch.int64):
            ii = ii.to(torch.int64)
        ext().embedding_bwd(ii, dout2d.contiguous(), dtable, n, bag, dim, avg)
        return
    g = dout2d.float() / (bag if avg else 1)
    ii = idx.long().reshape(-1)
    valid = (ii >= 0) & (ii < dtable.shape[0])
    dtable.index_add_(0, ii[valid], g.repeat_interleave(bag, 0)[valid])


# ----------------------------------------------------------------------------------- LSTM
def lstm_fwd_cell(G, ldg, c_prev, c_out, h_out, ldh, B, H):
    """One LSTM step in place on the gate rows G (pre-activations -> activated i, f, g, o), c_out
    (fp32) and h_out rows; G / h_out are row views with row strides ldg / ldh (elements)."""
    if native(G):
        ext().lstm_fwd_cell(G, ldg, c_prev, c_out, h_out, ldh, B, H)
        return
    g = G.as_strided((B, 4 * H), (ldg, 1))
    gf = g.float()
    i, f, gg, o = torch.sigmoid(gf[:, :H]), torch.sigmoid(gf[:, H:2 * H]), torch.tanh(gf[:, 2 * H:3 * H]), \
        torch.sigmoid(gf[:, 3 * H:])
    c = f * c_prev.view(B, H) + i * gg
    c_out.view(B, H).copy_(c)
    h_out.as_strided((B, H), (ldh, 1)).copy_((o * torch.tanh(c)).to(h_out.dtype))
    g.copy_(torch.cat([i, f, gg, o], 1).to(G.dtype))


def lstm_bwd_cell(G, ldg, c, c_prev, dy, lddy, dh_rec, dc, dG, B, H):
    """Backward of one step: pre-activation gate gradients into dG rows (may alias G), dc
    (fp32, in: dc_next, out: dc_prev). dy rows (stride lddy) and dh_rec [B, H] are optional."""
    if native(G):
        ext().lstm_bwd_cell(G, ldg, c, c_prev, dy, lddy, dh_rec, dc, dG, B, H)
        return
    g = G.as_strided((B, 4 * H), (ldg, 1)).float().clone()  # dG may alias G: read everything first
    i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
    dh = torch.zeros(B, H)
    if dy is not None:
        dh = dh + dy.as_strided((B, H), (lddy, 1)).float()
    if dh_rec is not None:
        dh = dh + dh_rec.view(B, H).float()
    tc = torch.tanh(c.view(B, H))
    dcv = dc.view(B, H) + dh * o * (1 - tc * tc)
    out = torch.cat([dcv * gg * i * (1 - i), dcv * c_prev.view(B, H) * f * (1 - f), dcv * i * (1 - gg * gg),
                     dh * tc * o * (1 - o)], 1)
    dG.as_strided((B, 4 * H), (ldg, 1)).copy_(out.to(dG.dtype))
    dc.view(B, H).copy_(dcv * f)


# ----------------------------------------------------------------------------- optimizers
GRAD_SUMSQ_PARTIALS = 2048  # fp32 workspace elements grad_sumsq needs (csrc: grad_sumsq_partials())


def grad_sumsq(x, partials, out, accumulate=False):
    """out (+)= sum of x**2 over a contiguous, 16-byte aligned fp32 range, in fp32, deterministic
    (no atomics: the same input gives the same bits). out: fp32 [1]; partials: fp32
    [GRAD_SUMSQ_PARTIALS] workspace the caller allocates once."""
    if native(x):
        ext().grad_sumsq(x, partials, out, bool(accumulate))
        return
    s = (x.float() * x.float()).sum(dtype=torch.float32)
    if accumulate:
        out.add_(s)
    else:
        out.fill_(s)


def clip_coef(sumsq, max_norm, norm, coef, eps=1e-6):
    """norm = sqrt(sumsq), coef = min(1, max_norm / (norm + eps)) (torch's clip_grad_norm_), all
    fp32 [1] on the device: the update kernels read coef through gscale_dev, with no host sync."""
    if native(sumsq):
        ext().clip_coef(sumsq, float(max_norm), norm, coef, float(eps))
        return
    norm.copy_(sumsq.sqrt())
    coef.copy_(torch.clamp(max_norm / (norm + eps), max=1.0))


def sgd_update(master, grad, mom, lowp, lr, momentum, nesterov, wd, gscale=1.0, max_blocks=0, gscale_dev=None):
    """max_blocks > 0 caps the launch grid (overlapped side-stream updates, Executor._on_bucket_ready).
    gscale_dev: optional one-element fp32 device tensor multiplied into gscale (the clipping
    coefficient of clip_coef); the weight-decay term is not scaled."""
    if native(master):
        ext().sgd_update(master, grad, mom, lowp, lr, momentum, nesterov, wd, gscale, max_blocks, gscale_dev)
        return
    if gscale_dev is not None:
        gscale = gscale * float(gscale_dev.item())
    g = grad * gscale + wd * master
    if momentum > 0:
        mom.mul_(momentum).add_(g)
        g = g + momentum * mom if nesterov else mom
    master.sub_(lr * g)
    if lowp is not None:
        lowp.copy_(master)


def sgd_sparse_rows(idx, mark, master, grad, lowp, lr):
    """master[r] -= lr * grad[r] (and the bf16 copy), then grad[r] = 0, for each distinct row r named
    in idx — plain SGD restricted to the rows a step touched (exact when momentum = weight decay =
    0: no other row has a non-zero gradient). Ids outside
    [0, rows) are ignored (other vocab-parallel parts' rows). mark: int32 [rows] scratch."""
    idx = idx.reshape(-1)
    if native(master):
        ext().sgd_sparse_rows(idx.to(torch.int64).contiguous(), mark, master, grad, lowp, lr)
        return
    rows = torch.unique(idx.to(torch.int64))
    rows = rows[(rows >= 0) & (rows < master.shape[0])]
    master[rows] -= lr * grad[rows]
    grad[rows] = 0
    if lowp is not None:
        lowp[rows] = master[rows].to(lowp.dtype)


def adam_update(master, grad, m, v, lowp, alpha_t, b1, b2, wd, eps, gscale=1.0, max_blocks=0, alpha_dev=None,
                gscale_dev=None):
    """alpha_dev: optional one-element fp32 device tensor the kernel reads the step size from (a
    captured training step replays the launch while alpha_t changes every step). gscale_dev: as in
    sgd_update."""
    if native(master):
        ext().adam_update(master, grad, m, v, lowp, alpha_t, b1, b2, wd, eps, gscale, max_blocks, alpha_dev,
                          gscale_dev)
        return
    if alpha_dev is not None:
        alpha_t = float(alpha_dev.item())
    if gscale_dev is not None:
        gscale = gscale * float(gscale_dev.item())
    _moments_(m, v, grad * gscale + wd * master, b1, b2)
    master.sub_(alpha_t * m / (v.sqrt() + eps))
    if lowp is not None:
        lowp.copy_(master)


# LAMB (csrc/kernels/optimizer.hip): two passes over a chunk table, one trust ratio per weight
LAMB_CHUNK = 8192  # most elements of one chunk = one workgroup (csrc: lamb_chunk())


class LambTable:
    """The chunk and weight tables of one arena and one set of update ranges, built once on the
    host (lamb_table) and uploaded once; the launches of a step read them from the device.
    chunks: int64 [n_chunks, 2] = (start, len | weight << 32); wtab: int32 [n_weights, 4] =
    (bits of lambda, flags, first chunk, chunk count), flags bit 0 = adapt, bit 1 = owned."""

    def __init__(self, chunks, wtab, size, device):
        self.chunks_host, self.wtab_host = chunks, wtab
        self.n_chunks, self.n_weights, self.size = int(chunks.shape[0]), int(wtab.shape[0]), int(size)
        self.chunks = torch.from_numpy(chunks).to(device)
        self.wtab = torch.from_numpy(wtab).to(device)

    def rows(self):
        """[(start, len, weight)] of the chunks, for the CPU fallbacks."""
        c = self.chunks_host
        return [(int(s), int(p & 0xFFFFFFFF), int(p >> 32)) for s, p in c]

    def lambdas(self):  # the per-weight lambdas as an fp32 CPU tensor [n_weights], for the CPU fallbacks
        return torch.from_numpy(self.wtab_host[:, 0].copy()).view(torch.float32)


def lamb_table(entries, ranges, n_weights, size, device, owned=()):
    """entries: [(offset, numel, weight, lambda, adapt)], one per weight of the arena, in arena
    order; ranges: the [lo, hi) element ranges this rank updates (the whole arena, or its ZeRO
    chunks). Each piece (entry x range) is cut into chunks of at most LAMB_CHUNK elements whose
    starts are 16-byte aligned; the padding between entries is in no chunk. Every entry's weight
    gets a row (with no chunks if no range meets it), and so does every weight index in `owned`
    (weights this rank holds no shard of: their norms are written as zeros). Misaligned or
    out-of-range input raises RuntimeError: the kernels trust the table."""
    import numpy as np
    size, n_weights = int(size), int(n_weights)
    rs = sorted((int(lo), int(hi)) for lo, hi in ranges)
    end = 0
    for lo, hi in rs:
        if lo % 4 or lo < end or hi < lo or hi > size:
            raise RuntimeError(f"lamb_table: range [{lo}, {hi}) is misaligned, overlapping or outside [0, {size})")
        end = hi
    wtab = np.zeros((n_weights, 4), dtype=np.int32)
    seen = set()
    chunks = []
    for off, n, wi, lam, adapt in entries:
        off, n, wi = int(off), int(n), int(wi)
        if off % 4 or off < 0 or n < 0 or off + n > size:
            raise RuntimeError(f"lamb_table: entry [{off}, {off + n}) is misaligned or outside [0, {size})")
        if not 0 <= wi < n_weights or wi in seen:
            raise RuntimeError(f"lamb_table: weight index {wi} is repeated or outside [0, {n_weights})")
        seen.add(wi)
        first = len(chunks)
        for lo, hi in rs:
            a, b = max(off, lo), min(off + n, hi)
            while a < b:
                ln = min(LAMB_CHUNK, b - a)
                chunks.append((a, ln | (wi << 32)))
                a += ln
        wtab[wi] = (np.float32(lam).view(np.int32), (1 if adapt else 0) | 2, first, len(chunks) - first)
    for wi in owned:
        if not 0 <= int(wi) < n_weights or int(wi) in seen:
            raise RuntimeError(f"lamb_table: weight index {wi} is repeated or outside [0, {n_weights})")
        seen.add(int(wi))
        wtab[int(wi)] = (0, 2, 0, 0)
    return LambTable(np.array(chunks, dtype=np.int64).reshape(-1, 2), wtab, size, device)


def _lamb_u(m, v, w, rc1, rc2, eps, lam):
    return (m * rc1) / ((v * rc2).sqrt() + eps) + lam * w


def _moments_(m, v, g, b1, b2):  # the Adam moments of the (scaled) gradient g, in place
    m.mul_(b1).add_((1 - b1) * g)
    v.mul_(b2).add_((1 - b2) * g * g)


def lamb_moments(master, grad, m, v, table, hyper, gscale_dev, b1, b2, eps, partials):
    """Stage 1 over the table's chunks: m, v updated in place from gscale_dev * grad, and per chunk
    (sum w^2, sum u^2) into partials [2 * n_chunks], u = m rc1 / (sqrt(v rc2) + eps) + lambda w.
    hyper: fp32 [3] = (lr, rc1, rc2) on the tensors' device. grad is never written."""
    if native(master):
        ext().lamb_moments(master, grad, m, v, table.chunks, table.wtab, hyper, gscale_dev, b1, b2, eps, partials)
        return
    gs = gscale_dev[0] if gscale_dev is not None else 1.0
    lam = table.lambdas()
    for i, (s, ln, wi) in enumerate(table.rows()):
        _moments_(m[s:s + ln], v[s:s + ln], grad[s:s + ln] * gs, b1, b2)
        w = master[s:s + ln]
        u = _lamb_u(m[s:s + ln], v[s:s + ln], w, hyper[1], hyper[2], eps, lam[wi])
        partials[2 * i] = (w * w).sum(dtype=torch.float32)
        partials[2 * i + 1] = (u * u).sum(dtype=torch.float32)


def lamb_norms(partials, table, count, norms):
    """norms[2p], norms[2p + 1] = each owned weight's chunk partials summed in index order; zeros
    when count is false (a replica another rank counts) or the weight has no chunk here."""
    if native(partials):
        ext().lamb_norms(partials, table.n_chunks, table.wtab, bool(count), norms)
        return
    for p, (_, flags, first, cnt) in enumerate(table.wtab_host):
        if flags & 2:
            part = partials[2 * first:2 * (first + cnt)].view(-1, 2) if count else partials[:0].view(-1, 2)
            norms[2 * p] = part[:, 0].sum(dtype=torch.float32)
            norms[2 * p + 1] = part[:, 1].sum(dtype=torch.float32)


def lamb_apply(master, m, v, lowp, table, hyper, eps, norms):
    """Stage 2: w -= lr * r_p * u with r_p = sqrt(norms[2p] / norms[2p + 1]) formed from the
    (all-reduced) norms where the weight adapts and both are > 0, else 1; u recomputed from the
    stored m, v, w; the bf16 copy written in the same pass."""
    if native(master):
        ext().lamb_apply(master, m, v, lowp, table.chunks, table.wtab, hyper, eps, norms)
        return
    lam = table.lambdas()
    for s, ln, wi in table.rows():
        wn, un = norms[2 * wi].sqrt(), norms[2 * wi + 1].sqrt()
        r = wn / un if (table.wtab_host[wi, 1] & 1) and wn > 0 and un > 0 else 1.0
        w = master[s:s + ln]
        w.sub_(hyper[0] * r * _lamb_u(m[s:s + ln], v[s:s + ln], w, hyper[1], hyper[2], eps, lam[wi]))
        if lowp is not None:
            lowp[s:s + ln].copy_(w)


def lamb_ref(w, g, m, v, entries, t, lr, b1, b2, eps, bias_correction=True, coef=1.0):
    """The LAMB step in float64, the oracle of the kernels and of the optimizer. w, g, m, v: flat
    tensors; entries as in lamb_table, several entries may share a weight index (shards of one
    weight: the norms run over all of them). Returns (w, m, v, norms [n, 2]) as new float64
    tensors, norms holding (sum w^2, sum u^2) per weight index; elements in no entry are copied."""
    w, g, m, v = (x.detach().cpu().double().clone() for x in (w, g, m, v))
    d1 = 1 - b1 ** t if bias_correction else 1.0
    d2 = 1 - b2 ** t if bias_correction else 1.0
    n_w = 1 + max((int(e[2]) for e in entries), default=-1)
    norms = torch.zeros(n_w, 2, dtype=torch.float64)
    us = []
    for off, n, wi, lam, adapt in entries:
        s = slice(int(off), int(off) + int(n))
        gp = coef * g[s]
        m[s] = b1 * m[s] + (1 - b1) * gp
        v[s] = b2 * v[s] + (1 - b2) * gp * gp
        u = (m[s] / d1) / ((v[s] / d2).sqrt() + eps) + lam * w[s]
        norms[wi, 0] += (w[s] ** 2).sum()
        norms[wi, 1] += (u ** 2).sum()
        us.append(u)
    for (off, n, wi, lam, adapt), u in zip(entries, us):
        s = slice(int(off), int(off) + int(n))
        wn, un = norms[wi, 0].sqrt(), norms[wi, 1].sqrt()
        r = wn / un if adapt and wn > 0 and un > 0 else 1.0
        w[s] = w[s] - lr * r * u
    return w, m, v, norms


# AdamW (csrc/kernels/optimizer.hip): LAMB with a trust ratio of 1, in one pass over the chunks
# [c0, c1) of a lamb_table (built with adapt=False): decoupled decay, lambda per weight
def adamw_update(master, grad, m, v, lowp, table, c0, c1, hyper, gscale_dev, b1, b2, eps, max_blocks=0):
    """m, v updated from gscale_dev * grad, then w -= lr * (m rc1 / (sqrt(v rc2) + eps) + lambda w)
    and the bf16 copy, over the table's chunks [c0, c1) only. hyper: fp32 [3] = (lr, rc1, rc2) on
    the tensors' device. grad is never written, nor is anything outside those chunks. max_blocks
    > 0 caps the launch grid (the chunks are then strode over); <= 0: one workgroup per chunk."""
    c0, c1 = int(c0), int(c1)
    if native(master):
        ext().adamw_update(master, grad, m, v, lowp, table.chunks, table.wtab, c0, c1, hyper, gscale_dev, b1, b2,
                           eps, max(int(max_blocks), 0))
        return
    if not 0 <= c0 <= c1 <= table.n_chunks:
        raise RuntimeError(f"adamw_update: chunks [{c0}, {c1}) outside the table's {table.n_chunks}")
    gs = gscale_dev[0] if gscale_dev is not None else 1.0
    lam = table.lambdas()
    for s, ln, wi in table.rows()[c0:c1]:
        _moments_(m[s:s + ln], v[s:s + ln], grad[s:s + ln] * gs, b1, b2)
        w = master[s:s + ln]
        w.sub_(hyper[0] * _lamb_u(m[s:s + ln], v[s:s + ln], w, hyper[1], hyper[2], eps, lam[wi]))
        if lowp is not None:
            lowp[s:s + ln].copy_(w)


def adamw_ref(w, g, m, v, entries, t, lr, b1, b2, eps, coef=1.0):
    """The AdamW step in float64 (torch.optim.AdamW with amsgrad=False, one decay per entry), the
    oracle of the kernel and of the optimizer. w, g, m, v: flat tensors; entries as in lamb_table
    (offset, numel, weight, lambda, adapt), adapt ignored. Returns (w, m, v) as new float64
    tensors; elements in no entry are copied."""
    w, g, m, v = (x.detach().cpu().double().clone() for x in (w, g, m, v))
    d1, d2 = 1 - b1 ** t, 1 - b2 ** t
    for off, n, _, lam, *_ in entries:
        s = slice(int(off), int(off) + int(n))
        gp = coef * g[s]
        m[s] = b1 * m[s] + (1 - b1) * gp
        v[s] = b2 * v[s] + (1 - b2) * gp * gp
        w[s] = w[s] - lr * ((m[s] / d1) / ((v[s] / d2).sqrt() + eps) + lam * w[s])
    return w, m, v


# ---------------------------------------------------------------------------- initializers
def _mix64(z):
    M = (1 << 64) - 1
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & M
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & M
    return z ^ (z >> 31)


def _u01_ref(seed, idx, stream):
    # same counter hash as csrc/kernels/init.hip, evaluated with int64 torch ops (wraparound)
    M = (1 << 64) - 1
    base = (seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019 + stream) & M
    z = idx.to(torch.int64) * 2
    z = z + _to_signed(base)

    def xshift(z, s):  # logical shift on 64-bit wrapped values
        return (z >> s) & ((1 << (64 - s)) - 1)

    z = (z ^ xshift(z, 30)) * _to_signed(0xBF58476D1CE4E5B9)
    z = (z ^ xshift(z, 27)) * _to_signed(0x94D049BB133111EB)
    z = z ^ xshift(z, 31)
    top = xshift(z, 40).to(torch.float64)
    return ((top + 0.5) / 16777216.0).to(torch.float32)


def _to_signed(u):
    return u - (1 << 64) if u >= (1 << 63) else u


def init_uniform(out, lo, hi, seed, offset=0):
    if native(out):
        ext().init_uniform(out, lo, hi, int(seed), int(offset))
        return
    idx = torch.arange(out.numel(), dtype=torch.int64) + int(offset)
    out.copy_((lo + (hi - lo) * _u01_ref(int(seed), idx, 0)).view(out.shape))


def init_normal(out, mean, std, seed, offset=0):
    if native(out):
        ext().init_normal(out, mean, std, int(seed), int(offset))
        return
    idx = torch.arange(out.numel(), dtype=torch.int64) + int(offset)
    a = _u01_ref(int(seed), idx, 0)
    b = _u01_ref(int(seed), idx, 1)
    r = torch.sqrt(-2 * torch.log(a)) * torch.cos(6.283185307179586 * b)
    out.copy_((mean + std * r).view(out.shape))


def fill(out, v):
    if native(out) and out.dtype in (torch.bfloat16, torch.float32):
        ext().fill(out, float(v))
    else:
        out.fill_(v)


def metrics_classify(probs2d, labels, acc3, ignore_index=None):
    """acc3 += {correct, sum CE, rows}; rows labelled ignore_index are left out of all three."""
    if native(probs2d):
        kw = {} if ignore_index is None else {"ignore_index": int(ignore_index)}
        ext().metrics_classify(probs2d.contiguous(), labels.contiguous(), probs2d.shape[0], probs2d.shape[1], acc3,
                               **kw)
        return
    p = probs2d.float()
    lab = labels.long()
    if ignore_index is not None:
        keep = lab != int(ignore_index)
        inr = keep & (lab >= 0) & (lab < p.shape[1])
        acc3[0] += ((p.argmax(-1) == lab) & keep).float().sum()
        pl = p.gather(1, lab.clamp(0, p.shape[1] - 1)[:, None])[:, 0]
        acc3[1] += torch.where(inr, -torch.log(pl.clamp_min(1e-12)), torch.zeros_like(pl)).sum()
        acc3[2] += keep.float().sum()
        return
    acc3[0] += (p.argmax(-1) == lab).float().sum()
    acc3[1] += -torch.log(p.gather(1, lab[:, None]).clamp_min(1e-12)).sum()
    acc3[2] += p.shape[0]


# ------------------------------------------------------------------ batch norm / pooling (NCHW / channel-last)
@torch.no_grad()
def batchnorm_fwd(x, g, b, run_mean, run_var, training, relu, eps=1e-5, momentum=0.1):
    """Spatial batch norm (+ReLU) of an NCHW tensor (csrc/kernels/cnn.hip). Training normalizes with
    the batch statistics and updates run_mean / run_var in place (unbiased variance, as torch);
    inference uses the running statistics. Returns (y, mean, rstd) for the backward."""
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(1, N * C)
    if native(x):
        nhwc = cl_ok(x, C)
        x = cl_dense(x, nhwc)
        y = torch.empty_like(x)
        mean = torch.empty(C, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        ws = torch.empty(ext().bn_ws(N, C, HW), device=x.device, dtype=torch.float32)
        ext().batchnorm_fwd(x, y, g, b, mean, rstd, run_mean, run_var, ws, N, C, HW, eps, momentum, training, relu,
                            nhwc)
        return y, mean, rstd
    xf = x.float().reshape(N, C, HW)
    if training:
        mean = xf.mean((0, 2))
        var = xf.var((0, 2), unbiased=False)
        n = N * HW
        run_mean.mul_(1 - momentum).add_(momentum * mean)
        run_var.mul_(1 - momentum).add_(momentum * var * (n / max(n - 1, 1)))
    else:
        mean, var = run_mean.clone(), run_var
    rstd = torch.rsqrt(var + eps)
    y = (xf - mean[None, :, None]) * rstd[None, :, None] * g.float()[None, :, None] + b.float()[None, :, None]
    if relu:
        y = y.clamp_min(0)
    return y.reshape(x.shape).to(x.dtype), mean, rstd


@torch.no_grad()
def batchnorm_bwd(x, dy, g, b, mean, rstd, dg, db, relu):
    """dx of batchnorm_fwd (training statistics); dg / db (fp32) += their per-channel sums."""
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(1, N * C)
    if native(x):
        nhwc = cl_ok(x, C)
        x = cl_dense(x, nhwc)
        dx = torch.empty_like(x)
        ws = torch.empty(ext().bn_ws(N, C, HW), device=x.device, dtype=torch.float32)
        ext().batchnorm_bwd(x, cl_dense(dy, nhwc), g, b, mean, rstd, dx, dg, db, ws, N, C, HW, relu, nhwc)
        return dx
    xf = x.float().reshape(N, C, HW)
    xh = (xf - mean[None, :, None]) * rstd[None, :, None]
    d = dy.float().reshape(N, C, HW)
    gf, bf = g.float()[None, :, None], b.float()[None, :, None]
    if relu:
        d = d * ((xh * gf + bf) > 0)
    s1, s2 = d.sum((0, 2)), (d * xh).sum((0, 2))
    m = N * HW
    dx = gf * rstd[None, :, None] * (d - s1[None, :, None] / m - xh * s2[None, :, None] / m)
    if dg is not None:
        dg.add_(s2)
    if db is not None:
        db.add_(s1)
    return dx.reshape(x.shape).to(x.dtype)


def pool_out_size(n, k, s, p0, p1):
    return (n + p0 + p1 - k) // s + 1


def _pool_ref(x, kh, kw, sh, sw, pads, is_max, include_pad, relu):
    pt, pb, pl, pr = pads
    if is_max:
        xp = F.pad(x, (pl, pr, pt, pb), value=float("-inf")) if any(pads) else x
        y = F.max_pool2d(xp, (kh, kw), (sh, sw))
    elif pt == pb and pl == pr:
        y = F.avg_pool2d(x, (kh, kw), (sh, sw), (pt, pl), count_include_pad=include_pad)
    else:  # asymmetric (spatially split block): window sums over the zero-padded block / divisor
        s = F.avg_pool2d(F.pad(x, (pl, pr, pt, pb)), (kh, kw), (sh, sw), 0, divisor_override=1)
        if include_pad:  # floor-sized windows never leave the padded extent: divisor kh * kw
            y = s / (kh * kw)
        else:
            ones = torch.ones_like(x[:1, :1])
            y = s / F.avg_pool2d(F.pad(ones, (pl, pr, pt, pb)), (kh, kw), (sh, sw), 0, divisor_override=1)
    return y.clamp_min(0) if relu else y


@torch.no_grad()
def pool2d_fwd(x, kh, kw, sh, sw, pads, is_max, include_pad, relu, need_idx):
    """2-D max / average pooling (+ReLU) of an NCHW tensor; pads = (top, bottom, left, right).
    Returns (y, idx): idx holds the winning window offset per output (max pooling, device)."""
    N, C, H, W = x.shape
    OH = pool_out_size(H, kh, sh, pads[0], pads[1])
    OW = pool_out_size(W, kw, sw, pads[2], pads[3])
    if native(x):
        nhwc = cl_ok(x, C)
        x = cl_dense(x, nhwc)
        y = torch.empty((N, C, OH, OW), device=x.device, dtype=x.dtype,
                        memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        idx = torch.empty(y.numel(), device=x.device, dtype=torch.uint8) if (is_max and need_idx) else None
        ext().pool2d_fwd(x, y, idx, [N, C, H, W, OH, OW, kh, kw, sh, sw, *pads], is_max, include_pad, relu, nhwc)
        return y, idx
    return _pool_ref(x.float(), kh, kw, sh, sw, pads, is_max, include_pad, relu).to(x.dtype), None


def pool2d_bwd(x, y, dy, idx, kh, kw, sh, sw, pads, is_max, include_pad, relu):
    """dx of pool2d_fwd (gather over the covering outputs; max pooling routes dy to the winners)."""
    N, C, H, W = x.shape
    if native(x):
        nhwc = cl_ok(x, C)  # the forward's decision: idx is in its output's memory order
        x = cl_dense(x, nhwc)
        dx = torch.empty_like(x)
        OH, OW = dy.shape[-2:]
        ext().pool2d_bwd(x, cl_dense(y, nhwc) if y is not None else None, cl_dense(dy, nhwc), idx, dx,
                         [N, C, H, W, OH, OW, kh, kw, sh, sw, *pads], is_max, include_pad, relu, nhwc)
        return dx
    xr = x.detach().float().requires_grad_()
    with torch.enable_grad():
        yr = _pool_ref(xr, kh, kw, sh, sw, pads, is_max, include_pad, relu)
    (dx,) = torch.autograd.grad(yr, (xr,), dy.detach().float())
    return dx.to(x.dtype)


# ------------------------------------------------------------------ convolution (NCHW / channel-last)
# Our implicit-GEMM MFMA kernels (csrc/kernels/conv.hip) and MIOpen (through torch) are both
# timed once per call site (geometry) outside graph capture and the faster one is kept, as for
# GEMMs; FF_CONV_IMPL=ours|lib forces one. The choices land in TUNE_LOG.
_conv_tuned: dict = {}
_CONV_IMPL = _os.environ.get("FF_CONV_IMPL", "")
_CONV_LIB_MARGIN = float(_os.environ.get("FF_CONV_LIB_MARGIN", "0.25"))


def conv_geometry(x, w, stride, pad, groups):
    N, C, H, W = x.shape
    K, _, KH, KW = w.shape
    OH = (H + 2 * pad[0] - KH) // stride[0] + 1
    OW = (W + 2 * pad[1] - KW) // stride[1] + 1
    return [N, C, H, W, K, OH, OW, KH, KW, stride[0], stride[1], pad[0], pad[1], groups]


@torch.no_grad()
def _conv_lib_fwd(x, w, b, g, relu):
    y = F.conv2d(x, w, b, (g[9], g[10]), (g[11], g[12]), 1, g[13])
    return torch.relu_(y) if relu else y


@torch.no_grad()
def _conv_lib_bwd(x, w, dy, g, need_dx, need_dw):
    dx, dw, _ = torch.ops.aten.convolution_backward(dy, x, w, None, [g[9], g[10]], [g[11], g[12]], [1, 1], False,
                                                    [0, 0], g[13], [need_dx, need_dw, False])
    return dx, dw


def _conv_ours_fwd(x, w, b, g, relu, y_nhwc, wpack_bwd=None):
    y = torch.empty((g[0], g[4], g[5], g[6]), device=x.device, dtype=x.dtype,
                    memory_format=torch.channels_last if y_nhwc else torch.contiguous_format)
    ws = torch.empty(ext().conv_ws(g), device=x.device, dtype=torch.bfloat16)
    ext().conv2d_fwd(x, w, b, y, ws, g, relu, _nhwc_flag(x, g[1] // g[13]), y_nhwc, wpack_bwd)
    return y


def _nhwc_flag(t, c):
    return cl_ok(t, c) and is_nhwc(t)


def _conv_ours_bwd(x, w, dy, g, dx_out, dw_out, accum_dx=False, wpack=None, dact=None):
    """dact = (y_p, db_p): the dgrad epilogue applies the producer's ReLU (y_p > 0) and adds the
    per-channel sums of the result into db_p (fp32, may be None) — see conv.hip IGemmArgs.dmask."""
    ws = torch.empty(ext().conv_ws(g), device=x.device, dtype=torch.bfloat16)
    dmask = dpart = None
    if dact is not None:
        dmask = dact[0]
        dpart = torch.empty(ext().conv_dact_rows(g) * g[1], device=x.device, dtype=torch.float32)
    ext().conv2d_bwd(x, w, dy, dx_out, dw_out, ws, g, _nhwc_flag(x, g[1] // g[13]), _nhwc_flag(dy, g[4] // g[13]),
                     accum_dx, wpack, dmask, dpart)
    if dact is not None and dact[1] is not None:
        ext().col_reduce_add3(dpart, dact[1].view(-1), None, None, ext().conv_dact_rows(g), g[1])


def _pointwise_gemm_ok(g, *ts):
    """A 1x1, stride-1, unpadded, ungrouped convolution over channel-last tensors is a plain GEMM
    over the N*H*W pixel rows: y[P][K] = x[P][C] . w[K][C]^T (csrc/kernels GEMMs, tuned per call
    site like any Linear)."""
    return (g[7] == 1 and g[8] == 1 and g[9] == 1 and g[10] == 1 and g[11] == 0 and g[12] == 0 and g[13] == 1
            and all(t is not None and is_nhwc(t) for t in ts))


def _rows(t):
    """[N][C][H][W] channel-last tensor -> its [N*H*W][C] row view."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _conv_gemm_fwd(x, w, b, g, relu):
    P, C, K_ = g[0] * g[5] * g[6], g[1], g[4]
    y = torch.empty((g[0], K_, g[5], g[6]), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    gemm(_rows(x), w.reshape(K_, C), _rows(y), P, K_, C, True, True, C, C, K_, bias=b,
         act=ACT_RELU if relu else ACT_NONE)
    return y


def _conv_gemm_bwd(x, w, dy, g, dx_out, dw_out, accum_dx=False):
    """dx[P][C] (+)= dy[P][K] . w[K][C];  dw[K][C] += dy^T . x (fp32)."""
    P, C, K_ = g[0] * g[5] * g[6], g[1], g[4]
    dyr = _rows(dy)
    if dx_out is not None:
        gemm(dyr, w.reshape(K_, C), _rows(dx_out), P, C, K_, True, False, K_, C, C, beta=1.0 if accum_dx else 0.0)
    if dw_out is not None:
        gemm(dyr, _rows(x), dw_out.view(K_, C), K_, C, P, False, False, K_, C, C, beta=1.0)


def _conv_pick(kind, key, cands):
    if _CONV_IMPL in ("ours", "lib"):
        return _CONV_IMPL
    if _CONV_IMPL == "gemm":
        return "gemm" if "gemm" in cands else "ours"
    choice = _conv_tuned.get((kind, key))
    if choice is None:
        choice = _tune_cache_lookup("conv", (kind, key))
        if choice is not None:
            _conv_tuned[(kind, key)] = choice
    if choice is None:
        if not _TUNE or torch.cuda.is_current_stream_capturing():
            return "ours"
        times = _time_all(cands, rounds=2)  # interleaved, best of 2 rounds: single passes flipped choices
        # MIOpen must win by _CONV_LIB_MARGIN (25 %): its timing in isolation leaves out the layout
        # copies and tensor ops around it in the step (Inception-v3 b64: per-site picks 14.17
        # ms/step, all ours 14.02, with MIOpen ahead by 1-20 % at its 12 sites;
        # profiles/conv_pick_ab_r4.txt)
        mine = min((k for k in times if k != "lib"), key=lambda k: times[k])
        choice = "lib" if times["lib"] < (1.0 - _CONV_LIB_MARGIN) * times[mine] else mine
        TUNE_LOG.append({"op": f"conv2d_{kind}", "geom": list(key), "times_ms": {k: round(v, 4) for k, v in
                                                                               times.items()}, "choice": choice})
        _conv_tuned[(kind, key)] = choice
    return choice


def _bwd_picks_ours(g, nhwc):
    """May this geometry's backward run our implicit-GEMM dgrad (its pick is "ours" or not made)?"""
    seen = [_conv_tuned.get(("bwd", tuple(g) + (True, dw, nhwc))) for dw in (True, False)]
    seen = [c for c in seen if c is not None]
    return _CONV_IMPL in ("", "ours") and (not seen or "ours" in seen)


def conv2d_fwd(x, w, b, stride, pad, groups, relu, bwd_pack=None):
    """y = [relu](conv2d(x, w) + b) (NCHW logical shapes). bf16 on the device: our implicit-GEMM
    kernel or MIOpen, whichever the per-geometry timing picked, with a channel-last output when
    CHANNELS_LAST (and the output channels per group are a multiple of 8); otherwise torch (fp32 /
    CPU reference). bwd_pack (a dict, training): our forward kernel also packs the backward-data
    weight operand in its pack launch and leaves it in bwd_pack["w"] for conv2d_bwd(wpack=...)."""
    g = conv_geometry(x, w, stride, pad, groups)
    if native(x) and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16:
        x = cl_dense(x, cl_ok(x, g[1] // groups))
        w = w.contiguous()
        b = b.contiguous() if b is not None else None
        y_nhwc = cl_ok(x, g[4] // groups)

        def lib():
            y = _conv_lib_fwd(x, w, b, g, relu)
            return cl_dense(y, y_nhwc)

        cands = {"ours": lambda: _conv_ours_fwd(x, w, b, g, relu, y_nhwc), "lib": lib}
        if y_nhwc and _pointwise_gemm_ok(g, x):
            cands["gemm"] = lambda: _conv_gemm_fwd(x, w, b, g, relu)
        choice = _conv_pick("fwd", tuple(g) + (is_nhwc(x),), cands)
        if choice == "gemm":
            return _conv_gemm_fwd(x, w, b, g, relu)
        if choice == "ours":
            wpb = None
            if bwd_pack is not None and _bwd_picks_ours(g, is_nhwc(x)) and not _pointwise_gemm_ok(g, x):
                wpb = torch.empty(ext().conv_wpack(g), device=x.device, dtype=torch.bfloat16)
                bwd_pack["w"] = wpb
            return _conv_ours_fwd(x, w, b, g, relu, y_nhwc, wpb)
        return lib()
    return _conv_lib_fwd(x, w, b, g, relu)


def conv2d_bwd(x, w, dy, g, dw, need_dx, dx_acc=None, wpack=None, dact=None):
    """Backward of conv2d_fwd for geometry g (conv_geometry): returns dx (or None) and adds the
    weight gradient into dw (fp32, shaped like w, may be None). dx_acc: an existing gradient of x
    that dx is added into (and returned): our dgrad kernel accumulates in its epilogue when dx_acc
    has x's memory layout, otherwise a separate add. wpack: the backward-data weight operand packed
    by this step's forward (conv2d_fwd bwd_pack), used by our dgrad kernel instead of a pack pass.
    dact = (y_p, db_p): x came from a bias + ReLU convolution whose only consumer this is; the
    returned dx is that producer's pre-activation gradient dx * (y_p > 0), and db_p (fp32, may be
    None) gets its per-channel sums — in our dgrad kernel's epilogue when that kernel runs on
    channel-last tensors, else by the separate mask + sum pass (Executor._plan_dact_fusion)."""
    if not need_dx:
        dx_acc = None
    if dact is not None:
        assert need_dx and dx_acc is None, "dact fusion needs a fresh dx"
        fused = _conv2d_bwd_dact(x, w, dy, g, dw, wpack, dact)
        if fused is not None:
            return fused
        dx = conv2d_bwd(x, w, dy, g, dw, need_dx, None, wpack)
        return conv_bias_relu_bwd(dx, dact[0], dact[1])
    if native(x) and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16:
        x = cl_dense(x, cl_ok(x, g[1] // g[13]))
        dy = cl_dense(dy, cl_ok(dy, g[4] // g[13]))
        w = w.contiguous()

        def ours():
            dxo = torch.empty_like(x) if need_dx else None
            dwo = torch.zeros(w.shape, device=w.device, dtype=torch.float32) if dw is not None else None
            _conv_ours_bwd(x, w, dy, g, dxo, dwo)
            return dxo, dwo

        cands = {"ours": ours, "lib": lambda: _conv_lib_bwd(x, w, dy, g, need_dx, dw is not None)}
        gemm_ok = _pointwise_gemm_ok(g, x, dy) and (dw is None or (dw.dtype == torch.float32 and dw.is_contiguous()))
        if gemm_ok:
            def gemm_c():
                dxo = torch.empty_like(x) if need_dx else None
                dwo = torch.zeros(w.shape, device=w.device, dtype=torch.float32) if dw is not None else None
                _conv_gemm_bwd(x, w, dy, g, dxo, dwo)
                return dxo, dwo
            cands["gemm"] = gemm_c
        choice = _conv_pick("bwd", tuple(g) + (need_dx, dw is not None, is_nhwc(x)), cands)
        if choice == "gemm" and gemm_ok:
            acc_in = dx_acc is not None and dx_acc.dtype == x.dtype and is_nhwc(dx_acc)
            dxo = dx_acc if acc_in else (torch.empty_like(x) if need_dx else None)
            _conv_gemm_bwd(x, w, dy, g, dxo, dw, acc_in)
            if dx_acc is not None and not acc_in:
                dx_acc.add_(dxo)
                return dx_acc
            return dxo
        if choice == "gemm":
            choice = "ours"
        if choice == "ours":
            acc_in = dx_acc is not None and dx_acc.dtype == x.dtype and is_nhwc(dx_acc) == is_nhwc(x) and \
                (dx_acc.is_contiguous() or is_nhwc(dx_acc))
            dxo = dx_acc if acc_in else (torch.empty_like(x) if need_dx else None)
            if dw is not None and dw.dtype == torch.float32 and dw.is_contiguous() and dw.shape == w.shape:
                _conv_ours_bwd(x, w, dy, g, dxo, dw, acc_in, wpack)  # the slab reduce adds into the gradient
            else:
                dwo = torch.zeros(w.shape, device=w.device, dtype=torch.float32) if dw is not None else None
                _conv_ours_bwd(x, w, dy, g, dxo, dwo, acc_in, wpack)
                if dw is not None:
                    dw.add_(dwo.view_as(dw))
            if dx_acc is not None and not acc_in:
                dx_acc.add_(dxo)
                return dx_acc
            return dxo
    dxo, dwo = _conv_lib_bwd(x, w, dy, g, need_dx, dw is not None)
    if dw is not None:
        dw.add_(dwo.float().view_as(dw))
    if dx_acc is not None:
        dx_acc.add_(dxo)
        return dx_acc
    return dxo


def _conv2d_bwd_dact(x, w, dy, g, dw, wpack, dact):
    """The fused form of conv2d_bwd(dact=...) when our dgrad kernel serves this geometry on
    channel-last x / y_p (the per-site pick chose "ours"); None otherwise."""
    yp, dbp = dact
    if not (native(x) and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16):
        return None
    cg = g[1] // g[13]
    # the same predicate conv2d_bwd's x_nhwc flag is built from (_nhwc_flag): the C++ side applies
    # the mask only on that path and refuses a dmask otherwise
    if not (_nhwc_flag(x, cg) and is_nhwc(yp)) or yp.shape != x.shape or yp.dtype != torch.bfloat16:
        return None
    if dbp is not None and (dbp.dtype != torch.float32 or dbp.numel() != g[1]):
        return None
    pick = _CONV_IMPL if _CONV_IMPL in ("ours", "lib") else _conv_tuned.get(("bwd", tuple(g) + (True, dw is not None, True)))
    if pick != "ours":
        return None  # not timed yet (the unfused step times it), or the GEMM / library form won
    dy = cl_dense(dy, cl_ok(dy, g[4] // g[13]))
    w = w.contiguous()
    dxo = torch.empty_like(x)
    if dw is not None and dw.dtype == torch.float32 and dw.is_contiguous() and dw.shape == w.shape:
        _conv_ours_bwd(x, w, dy, g, dxo, dw, False, wpack, dact)
    else:
        dwo = torch.zeros(w.shape, device=w.device, dtype=torch.float32) if dw is not None else None
        _conv_ours_bwd(x, w, dy, g, dxo, dwo, False, wpack, dact)
        if dw is not None:
            dw.add_(dwo.view_as(dw))
    return dxo


@torch.no_grad()
def conv_bias_relu_bwd(dy, y, db):
    """NCHW: dz = dy masked by y > 0 when y is given (the fused ReLU), else dy; db (fp32, may be
    None) += per-channel sums of dz over (n, h, w)."""
    N, C = dy.shape[0], dy.shape[1]
    HW = dy.numel() // max(1, N * C)
    if y is None and db is None:
        return dy
    if native(dy):
        nhwc = cl_ok(dy, C)
        dy = cl_dense(dy, nhwc)
        dz = torch.empty_like(dy) if y is not None else None
        ws = torch.empty(ext().bn_ws(N, C, HW), device=dy.device, dtype=torch.float32)
        if db is not None and nhwc and _FOLDQ["on"]:  # the bias fold joins the batched folds
            X = ext()
            X.fold_record(True)
            try:
                X.channel_sum(dy, cl_dense(y, nhwc) if y is not None else None, dz, db, ws, N, C, HW, nhwc)
            finally:
                X.fold_record(False)
            _FOLDQ["keep"].append((ws, db))
            return dz if dz is not None else dy
        ext().channel_sum(dy, cl_dense(y, nhwc) if y is not None else None, dz, db, ws, N, C, HW, nhwc)
        return dz if dz is not None else dy
    dz = dy * (y > 0) if y is not None else dy
    if db is not None:
        db.add_(dz.float().reshape(N, C, HW).sum((0, 2)))
    return dz


# ------------------------------------------------------------------ RMS norm
@torch.no_grad()
def rmsnorm_fwd(x2d, w, eps):
    """y = x * rsqrt(mean(x^2) + eps) * w per row. Returns (y, rstd)."""
    rows, d = x2d.shape
    if native(x2d):
        y = torch.empty_like(x2d)
        rstd = torch.empty(rows, device=x2d.device, dtype=torch.float32)
        ext().rmsnorm_fwd(x2d, w, y, rstd, rows, d, eps)
        return y, rstd
    xf = x2d.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1) + eps)
    return (xf * rstd[:, None] * w.float()).to(x2d.dtype), rstd


@torch.no_grad()
def rmsnorm_bwd(x2d, w, dy2d, rstd, dw):
    """dx of rmsnorm_fwd; dw (fp32, may be None) += sum over rows of dy * x * rstd."""
    rows, d = x2d.shape
    if native(x2d):
        dx = torch.empty_like(x2d)
        ext().rmsnorm_bwd(x2d, w, dy2d, rstd, dx, dw, rows, d)
        return dx
    xf, dyf, r = x2d.float(), dy2d.float(), rstd[:, None]
    g = dyf * w.float()
    dx = r * g - (r ** 3) * xf * (g * xf).sum(-1, keepdim=True) / d
    if dw is not None:
        dw.add_((dyf * xf * r).sum(0))
    return dx.to(x2d.dtype)


# ------------------------------------------------------------------ mixture of experts (moe.hip)
MOE_MAX_EXPERTS = 64


def moe_on_device(t: torch.Tensor, n: int = 1) -> bool:
    """The HIP routing kernels run for bf16 / fp32 device tensors and up to 64 experts."""
    return native(t) and t.dtype in (torch.bfloat16, torch.float32) and n <= MOE_MAX_EXPERTS


def topk(x: torch.Tensor, k: int):
    """(values, int32 indices) of the k largest along the last dim, values descending (ties:
    lowest index first) — csrc/kernels/moe.hip, one wave per row."""
    xc = x.contiguous()
    vals = torch.empty(tuple(x.shape[:-1]) + (k,), device=x.device, dtype=x.dtype)
    idx = torch.empty(vals.shape, device=x.device, dtype=torch.int32)
    ext().topk_fwd(xc, vals, idx, k)
    return vals, idx


def topk_bwd(dvals: torch.Tensor, idx: torch.Tensor, shape) -> torch.Tensor:
    dx = torch.empty(shape, device=dvals.device, dtype=dvals.dtype)
    ext().topk_bwd(dvals.contiguous(), idx.contiguous(), dx)
    return dx


def moe_route(assign: torch.Tensor, n: int, cap: int):
    """Device routing of the B*k (sample, choice) pairs: (expert id, row in the expert's tensor or
    -1 when dropped past the capacity, load per expert), in the reference's sample order."""
    a = assign.reshape(-1).to(torch.int32).contiguous()
    L = a.numel()
    expert = torch.empty(L, device=a.device, dtype=torch.int32)
    pos = torch.empty(L, device=a.device, dtype=torch.int32)
    load = torch.empty(n, device=a.device, dtype=torch.int32)
    ws = torch.empty(max(1, int(ext().moe_route_ws_ints(L, n))), device=a.device, dtype=torch.int32)
    ext().moe_route(a, n, cap, expert, pos, load, ws)
    return expert, pos, load


# ------------------------------------------------------------------ fp32 attention (our kernels)
def attn_f32_supported(x) -> bool:
    return native(x) and x.dtype == torch.float32


def _kv_expand(t, st, b, Hkv, G, S, d):
    """Sample b of a flat K / V buffer of Hkv heads (strides st) with every head repeated G times:
    flat [Hkv * G, S, d], and its (head, row) strides."""
    view = t[b * st[0]:].as_strided((Hkv, S, d), (st[1], st[2], 1))
    return view.repeat_interleave(G, 0).reshape(-1), S * d, d


def attn_f32_fwd(q, qs, k, ks, v, vs, o, os_, B, H, Sq, Sk, kd, vd, scale, causal, key_lens=None, drop=None,
                 bias=None, segments=None, Hkv=None):
    """fp32 attention on our kernels, per sample: S = Q.K^T (f32 MFMA GEMM, heads as the batch),
    causal mask, key-length mask (key_lens: int32 [B] on the device, columns >= key_lens[b] set to
    -inf there), row softmax(scale * S) (softmax.hip), the same columns of P set to 0 (a sample of
    length 0 has P = 0, not the softmax's NaN), O = P.V. q/k/v/o are flat views with [b, h, row] element strides (qs, ks, vs, os_) and contiguous head dims.
    drop (as in flash_attn_fwd): the PV GEMM takes keep ? P / (1 - p_eff) : 0 (attn_dropout_f32 on P[b]);
    the P returned is the undropped one, for softmax_bwd.
    bias (attn_score_bias): S = scale * S + bias[b] (score_bias_f32) ahead of the masks, the softmax then
    runs with scale 1; P is set to 0 where S is -inf, so a row with no key left has P = 0.
    segments (attn_segments): S is set to -inf outside the query's run (segment_mask_f32) and P to 0
    there, so a padding row has P = 0.
    Hkv (attn_kv_heads): k / v hold Hkv heads; each sample's K / V are expanded to H heads for the GEMMs.
    Returns P [B, H, Sq, Sk]."""
    X = ext()
    Hkv = attn_kv_heads(H, Hkv)
    G = H // Hkv
    dkw = _drop_kw(drop)
    skw = _seg_kw(segments, key_lens, bias, Sq, Sk)
    bias = attn_score_bias(bias, B, H, Sq, Sk, q.device)
    if bias is not None:
        bflat, bsb = bias.reshape(-1), (bias.shape[1] * Sq * Sk if bias.shape[0] > 1 else 0)
        bsh = Sq * Sk if bias.shape[1] > 1 else 0
    Pd = torch.empty(H, Sq, Sk, device=q.device, dtype=torch.float32) if dkw else None
    key_lens = attn_key_lens(key_lens, B, q.device)
    q, k, v, o = q.reshape(-1), k.reshape(-1), v.reshape(-1), o.reshape(-1)
    P = torch.empty(B, H, Sq, Sk, device=q.device, dtype=torch.float32)
    S = torch.empty(H, Sq, Sk, device=q.device, dtype=torch.float32)
    for b in range(B):
        kb, ksh, kss = (k[b * ks[0]:], ks[1], ks[2]) if G == 1 else _kv_expand(k, ks, b, Hkv, G, Sk, kd)
        vb, vsh, vss = (v[b * vs[0]:], vs[1], vs[2]) if G == 1 else _kv_expand(v, vs, b, Hkv, G, Sk, vd)
        X.gemm_f32(q[b * qs[0]:], kb, S, None, None, Sq, Sk, kd, qs[2], kss, Sk, qs[1], ksh, Sq * Sk,
                   H, True, True, 1.0, 0.0, ACT_NONE)
        if bias is not None:
            X.score_bias_f32(S, bflat[b * bsb:], H, Sq, Sk, bsh, scale)
        if causal:
            X.causal_mask_f32(S, Sq, Sk)
        if key_lens is not None:
            X.key_len_mask_f32(S, key_lens, b, Sk, float("-inf"))
        if skw:
            X.segment_mask_f32(S, skw["seg_lo"], skw["seg_hi"], b, H, Sq, Sk)
        X.softmax_fwd(S, P[b], H * Sq, Sk, 1.0 if bias is not None else scale)
        if bias is not None or skw:
            X.masked_prob_zero_f32(P[b], S)
        if key_lens is not None:  # a sample without keys: its all -inf rows came out NaN, P is 0 there
            X.key_len_mask_f32(P[b], key_lens, b, Sk, 0.0)
        Pb = P[b]
        if dkw:
            X.attn_dropout_f32(P[b], Pd, H, Sq, Sk, dkw["b0"] + b, dkw["h0"], dkw["H_total"], dkw["drop_thr"],
                               dkw["rng_step"], dkw["rng_seed"])
            Pb = Pd
        X.gemm_f32(Pb, vb, o[b * os_[0]:], None, None, Sq, vd, Sk, Sk, vss, os_[2], Sq * Sk, vsh,
                   os_[1], H, True, False, 1.0, 0.0, ACT_NONE)
    return P


def attn_f32_bwd(q, qs, k, ks, v, vs, do, dos, P, dq, dk, dv, B, H, Sq, Sk, kd, vd, scale, key_lens=None, drop=None,
                 bias=None, segments=None, Hkv=None):
    """Backward of attn_f32_fwd: dP = dO.V^T, dS = scale * P * (dP - rowsum(dP * P)), dQ = dS.K,
    dK = dS^T.Q, dV = P^T.dO (dq / dk / dv share q / k / v's strides). key_lens needs no work here:
    the forward left P = 0 in the masked columns, so dS is 0 there and the dK / dV rows at or past a
    sample's length come out as zeros (all of a length-0 sample's gradients do). drop (with the
    counter value of the forward): dP and the P of the dV GEMM go through attn_dropout_f32. bias needs
    no work either: it is inside P, dS = scale * P * (..) stays the gradient of the raw q.k, and the
    bias itself takes no gradient. segments need none: P is 0 outside the runs. Hkv (as in attn_f32_fwd):
    dK / dV of the H query heads go to a per-sample buffer and each group's sum to dk / dv."""
    X = ext()
    Hkv = attn_kv_heads(H, Hkv)
    G = H // Hkv
    if G > 1:
        dkx = torch.empty(H, Sk, kd, device=q.device, dtype=torch.float32)
        dvx = torch.empty(H, Sk, vd, device=q.device, dtype=torch.float32)
    dkw = _drop_kw(drop)
    Pd = torch.empty(H, Sq, Sk, device=q.device, dtype=torch.float32) if dkw else None
    q, k, v, do = q.reshape(-1), k.reshape(-1), v.reshape(-1), do.reshape(-1)
    dq, dk, dv = dq.reshape(-1), dk.reshape(-1), dv.reshape(-1)
    dP = torch.empty(H, Sq, Sk, device=q.device, dtype=torch.float32)
    dS = torch.empty_like(dP)
    for b in range(B):
        kb, ksh, kss = (k[b * ks[0]:], ks[1], ks[2]) if G == 1 else _kv_expand(k, ks, b, Hkv, G, Sk, kd)
        vb, vsh, vss = (v[b * vs[0]:], vs[1], vs[2]) if G == 1 else _kv_expand(v, vs, b, Hkv, G, Sk, vd)
        dkb, dvb = (dk[b * ks[0]:], dv[b * vs[0]:]) if G == 1 else (dkx.view(-1), dvx.view(-1))
        X.gemm_f32(do[b * dos[0]:], vb, dP, None, None, Sq, Sk, vd, dos[2], vss, Sk, dos[1], vsh,
                   Sq * Sk, H, True, True, 1.0, 0.0, ACT_NONE)
        Pb = P[b]
        if dkw:
            da = (H, Sq, Sk, dkw["b0"] + b, dkw["h0"], dkw["H_total"], dkw["drop_thr"], dkw["rng_step"], dkw["rng_seed"])
            X.attn_dropout_f32(dP, dP, *da)
            X.attn_dropout_f32(P[b], Pd, *da)
            Pb = Pd
        X.softmax_bwd(P[b], dP, dS, H * Sq, Sk, scale, False)
        X.gemm_f32(dS, kb, dq[b * qs[0]:], None, None, Sq, kd, Sk, Sk, kss, qs[2], Sq * Sk, ksh,
                   qs[1], H, True, False, 1.0, 0.0, ACT_NONE)
        X.gemm_f32(dS, q[b * qs[0]:], dkb, None, None, Sk, kd, Sq, Sk, qs[2], kss, Sq * Sk, qs[1],
                   ksh, H, False, False, 1.0, 0.0, ACT_NONE)
        X.gemm_f32(Pb, do[b * dos[0]:], dvb, None, None, Sk, vd, Sq, Sk, dos[2], vss, Sq * Sk,
                   dos[1], vsh, H, False, False, 1.0, 0.0, ACT_NONE)
        if G > 1:
            for g, gx, st, d in ((dk, dkx, ks, kd), (dv, dvx, vs, vd)):
                g[b * st[0]:].as_strided((Hkv, Sk, d), (st[1], st[2], 1)).copy_(gx.view(Hkv, G, Sk, d).sum(1))
