"""Attention logit soft cap (Gemma-2) on the HIP decode, prefill and cached-context kernels against an fp64 NumPy restatement of
    logit(i, j) = c * tanh(scale * (q_i . k_j) / c) + alibi_slope * (j - i)     then mask, softmax, P.V
Tolerance: the project's bar (test_ops_gpu.py test_paged_attention): atol 1e-3 (FP8 KV 1e-2) + 2^-8 max|ref| for bf16, rtol 1e-5.
The queries are scaled (x40 for cap 50, x8 for cap 1) so that the fp64 reference with and without the cap differ by more than 100 x
the tolerance on every case (asserted): a kernel that ignores the cap fails.  |V| < 1 keeps the 16-bit output rounding under the bar."""
import functools

import numpy as np
import pytest
import torch

from oracle import attention as oa
from oracle import fp8 as of8

pytestmark = pytest.mark.gpu
DEV = "cuda"
Q_MUL = {1.0: 8.0, 50.0: 40.0}
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
# rnd: fp32 values rounded to the 16-bit type (what the kernels are handed), a CPU tensor; f64: back to numpy; dev: to the GPU
rnd = lambda x, dtype: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype)
f64 = lambda x: x if isinstance(x, np.ndarray) else x.float().numpy().astype(np.float64)
dev = lambda a, ty=np.int32: torch.from_numpy(np.asarray(a, ty)).to(DEV)
cat = lambda a, b: np.concatenate([f64(a), f64(b)])


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from aphrodite_engine_amd import _custom_ops, _lib
    _lib.lib()
    return _custom_ops


def refs(seqs, scale, cap, left=None, slopes=None):
    """seqs: (q [n,Hq,D] at key positions qpos0 + i, k, v [L,Hkv,D], qpos0); keys qpos - left .. qpos visible -> fp64 reference with / without cap"""
    out = []
    for c in (cap, 0.0):
        parts = []
        for q, k, v, qpos0 in seqs:
            q, k, v = f64(q), f64(k), f64(v)
            rep = q.shape[1] // k.shape[1]
            lg = scale * np.einsum("qhd,khd->hqk", q, np.repeat(k, rep, axis=1))
            lg = c * np.tanh(lg / c) if c else lg
            qpos, kpos = qpos0 + np.arange(q.shape[0])[:, None], np.arange(k.shape[0])[None, :]
            if slopes is not None:
                lg = lg + np.asarray(slopes, np.float64)[:, None, None] * (kpos - qpos)[None]
            lg = np.where(((kpos > qpos) | (False if left is None else qpos - kpos > left))[None], -np.inf, lg)
            p = np.exp(lg - lg.max(axis=2, keepdims=True))
            parts.append(np.einsum("hqk,khd->qhd", p / p.sum(axis=2, keepdims=True), np.repeat(v, rep, axis=1)))
        out.append(np.concatenate(parts))
    return out


def check(got, ref_pair, dtype, fp8=False):
    ref, ref_nocap = ref_pair
    atol = (1e-2 if fp8 else 1e-3) + (2.0 ** -8 * float(np.abs(ref).max()) if dtype == torch.bfloat16 else 0.0)
    assert np.abs(ref - ref_nocap).max() > 100 * atol, "the cap does not bite on these inputs"
    np.testing.assert_allclose(got.float().cpu().numpy(), ref, atol=atol, rtol=1e-5)


def qkv(rng, T, Hq, Hkv, D, dtype, mul):      # q ~ N(0, mul^2), k ~ N(0, 1), |v| < 1
    return (rnd(rng.standard_normal((T, Hq, D)) * mul, dtype), rnd(rng.standard_normal((T, Hkv, D)), dtype),
            rnd(rng.random((T, Hkv, D)) * 2 - 1, dtype))


def paged(rng, lens, room, Hkv, D, BS, dtype, kv):
    """Random paged cache (K ~ N(0, 1), |V| < 1; fp8: stored with scale 1, read with 0.7 / 1.3) -> kc, vc, tables, (K, V) of lens[i] tokens, scales"""
    bps, x = (room + BS - 1) // BS, 8 if kv == "auto" else 16
    NB = len(lens) * bps + 3
    kf, vf = rng.standard_normal((NB, Hkv, D // x, BS, x)).astype(np.float32), (rng.random((NB, Hkv, D, BS)) * 2 - 1).astype(np.float32)
    if kv == "auto":
        kc, vc, ks, vs = rnd(kf, dtype), rnd(vf, dtype), 1.0, 1.0
        knp, vnp = kc.float().numpy(), vc.float().numpy()
    else:
        knp, vnp, ks, vs = of8.kv_quant(kf, 1.0, kv), of8.kv_quant(vf, 1.0, kv), 0.7, 1.3
        kc, vc = torch.from_numpy(knp), torch.from_numpy(vnp)
    bt = rng.permutation(NB)[:len(lens) * bps].reshape(len(lens), bps).astype(np.int32)
    hist = [[a.astype(np.float64) for a in oa.gather_kv(knp, vnp, bt[i], L, kv, ks, vs)] for i, L in enumerate(lens)]
    return kc.to(DEV), vc.to(DEV), bt, hist, ks, vs


DECODE_CASES = {   # (Hq, Hkv, D, BS), lengths
    "edges": ((8, 2, 128, 16), [1, 513, 700]),      # one token, a partition edge, a tail; v1: the split form
    "hd256": ((4, 2, 256, 16), [173, 300]),
    "gqa32": ((32, 1, 128, 16), [77, 600]),         # second head pass
}


@functools.lru_cache(maxsize=None)
def decode_inputs(name, dt, kv, cap, alibi):
    (Hq, Hkv, D, BS), lens = DECODE_CASES[name]
    rng = np.random.default_rng([Hq, D, int(cap)])
    kc, vc, bt, hist, ks, vs = paged(rng, lens, max(lens), Hkv, D, BS, DTYPES[dt], kv)
    q = qkv(rng, len(lens), Hq, Hkv, D, DTYPES[dt], Q_MUL[cap])[0]
    slopes = (rng.standard_normal(Hq) * 0.05).astype(np.float32) if alibi else None
    args = (q.to(DEV), kc, vc, Hkv, D ** -0.5, dev(bt), dev(lens), BS, max(lens), None if slopes is None else dev(slopes, np.float32),
            kv, ks, vs)
    return args, refs([(q[i:i + 1], *hist[i], L - 1) for i, L in enumerate(lens)], D ** -0.5, cap, slopes=slopes)


@pytest.mark.parametrize("name,version,dt,kv,cap,alibi",
                         [(n, ver, dt, "auto", c, False) for n in DECODE_CASES for ver in ("v1", "v2", "rocm") for dt in DTYPES for c in Q_MUL]
                         + [("edges", ver, "f16", "fp8", c, False) for ver in ("v1", "v2") for c in Q_MUL]
                         + [("edges", "v2", "bf16", "auto", 50.0, True)])
def test_decode_softcap(ops, monkeypatch, name, version, dt, kv, cap, alibi):
    args, ref_pair = decode_inputs(name, dt, kv, cap, alibi)
    (S, Hq, D), P = args[0].shape, (args[8] + 511) // 512
    out = torch.full((S, Hq, D), float("nan"), dtype=DTYPES[dt], device=DEV)
    es, ml, tmp = (torch.full((S, Hq, P) + e, float("nan"), dtype=t, device=DEV) for e, t in (((), None), ((), None), ((D, ), DTYPES[dt])))
    if version == "v1":
        ops.paged_attention_v1(out, *args, softcap=cap)
    elif version == "v2":
        ops.paged_attention_v2(out, es, ml, tmp, *args, softcap=cap)
    else:
        monkeypatch.setenv("APHRO_PA_ROCM_PARTITIONED", "1")     # (without it the rocm op takes the v1 form at these sizes)
        ops.paged_attention_rocm(out, es, ml, tmp, *args, softcap=cap)
    check(out, ref_pair, DTYPES[dt], fp8=kv != "auto")
    if version != "v1" and P > 1 and not alibi:      # the scratch holds CAPPED logits: none above the cap
        assert 0.5 * cap < np.nanmax(ml.cpu().numpy()) <= cap * (1 + 1e-5)


def test_softcap_zero_is_the_uncapped_kernel_and_head_96_is_refused(ops):
    args = decode_inputs("edges", "f16", "auto", 1.0, False)[0]
    a, b = torch.empty_like(args[0]), torch.empty_like(args[0])
    ops.paged_attention_v1(a, *args)
    ops.paged_attention_v1(b, *args, softcap=0.0)
    assert torch.equal(a, b)
    q96 = torch.zeros(1, 4, 96, dtype=torch.float16, device=DEV)
    kc96, vc96 = torch.zeros(2, 1, 12, 16, 8, dtype=torch.float16, device=DEV), torch.zeros(2, 1, 96, 16, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="128"):
        ops.paged_attention_v1(torch.empty_like(q96), q96, kc96, vc96, 1, 0.1, dev([[1]]), dev([1]), 16, 1, None, "auto", 1.0, 1.0, softcap=50.0)
    with pytest.raises(RuntimeError, match="128"):
        ops.flash_attn_varlen(q96, q96[:, :1], q96[:, :1], dev([0, 1]), 1, 0.1, softcap=50.0)


@functools.lru_cache(maxsize=None)
def prefill_inputs(lens, D, dt, cap, left, alibi):
    rng = np.random.default_rng([D, int(cap), len(lens)])
    q, k, v = qkv(rng, sum(lens), 4, 2, D, DTYPES[dt], Q_MUL[cap])
    slopes = (rng.standard_normal(4) * 0.05).astype(np.float32) if alibi else None
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ref_pair = refs([(q[s:e], k[s:e], v[s:e], 0) for s, e in zip(cu[:-1], cu[1:])], D ** -0.5, cap, left, slopes)
    kw = dict(causal=True, window_size=None if left is None else (left, left), alibi_slopes=None if slopes is None else dev(slopes, np.float32))
    return (q.to(DEV), k.to(DEV), v.to(DEV), dev(cu), max(lens), D ** -0.5), kw, ref_pair


@pytest.mark.parametrize("left,cap,alibi", [(None, 1.0, False), (None, 50.0, False), (48, 1.0, False), (48, 50.0, False), (None, 50.0, True)])
@pytest.mark.parametrize("D,dt", [(128, "f16"), (128, "bf16"), (256, "f16"), (256, "bf16")])
@pytest.mark.parametrize("lens", [(1, 63, 64, 65, 200), (520, 77), (1100, )])   # generation 1; 2 (512+ rows, hd 128); 4 (knob lowered, hd 128)
def test_prefill_softcap(ops, lens, D, dt, left, cap, alibi):
    args, kw, ref_pair = prefill_inputs(lens, D, dt, cap, left, alibi)
    with ops.knob("APHRO_FA_V4_MIN_KEYS", 1024 if max(lens) >= 1024 else None):
        check(ops.flash_attn_varlen(*args, softcap=cap, **kw), ref_pair, DTYPES[dt])
    if cap == 1.0:
        assert torch.equal(ops.flash_attn_varlen(*args, **kw), ops.flash_attn_varlen(*args, softcap=0.0, **kw))


@pytest.mark.parametrize("cap", [1.0, 50.0])
@pytest.mark.parametrize("kv", ["auto", "fp8"])
@pytest.mark.parametrize("ctx,new", [((0, 17, 130), (5, 64, 33)), ((40, 3), (130, 20))])   # second: 128+ rows, second generation
def test_context_softcap(ops, ctx, new, kv, cap):
    rng = np.random.default_rng([len(ctx), int(cap)])
    Hq, Hkv, D, BS, scale, dtype = 4, 2, 128, 16, 0.07, torch.float16
    lens = [c + n for c, n in zip(ctx, new)]
    kc, vc, bt, hist, ks, vs = paged(rng, ctx, max(lens), Hkv, D, BS, dtype, kv)
    q, k, v = qkv(rng, sum(new), Hq, Hkv, D, dtype, Q_MUL[cap] / (scale * D ** 0.5))     # the logit spread of scale D^-0.5
    start = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    # the gather leaves the dequantised context in the query dtype (include/aphrodite_mi355x.h)
    seqs = [(q[s:e], cat(rnd(hk, dtype), k[s:e]), cat(rnd(hv, dtype), v[s:e]), c) for s, e, (hk, hv), c in zip(start[:-1], start[1:], hist, ctx)]
    out = torch.full_like(q, float("nan"), device=DEV)
    ops.context_attention_fwd(q.to(DEV), k.to(DEV), v.to(DEV), out, kv, kc, vc, dev(bt), dev(start), dev(lens), dev(ctx), max(new), ks, vs,
                              scale=scale, softcap=cap)
    check(out, refs(seqs, scale, cap), dtype, fp8=kv != "auto")


@pytest.mark.parametrize("max_context_len", [None, 0])      # None: the prefill goes through forward_prefix; 0: through flash_attn_varlen
def test_backend_forward_with_logits_soft_cap(ops, max_context_len):
    from aphrodite_engine_amd.attention import MI355XAttentionImpl, MI355XAttentionMetadata
    rng = np.random.default_rng(21)
    Hq, Hkv, D, BS, cap, scale, dtype = 8, 2, 128, 16, 50.0, 0.07, torch.float16
    plens, dlens = [40, 17], [23, 70]                          # decode lengths include the new token
    kc, vc, bt, hist, _, _ = paged(rng, [0, 0, dlens[0] - 1, dlens[1] - 1], 80, Hkv, D, BS, dtype, "auto")
    kv_cache = torch.stack([kc.reshape(kc.shape[0], -1), vc.reshape(vc.shape[0], -1)])
    npf = sum(plens)
    q, k, v = qkv(rng, npf + 2, Hq, Hkv, D, dtype, Q_MUL[cap] / (scale * D ** 0.5))
    slot = lambda si, p: int(bt[si, p // BS]) * BS + p % BS
    slots = [slot(si, p) for si, L in enumerate(plens) for p in range(L)] + [slot(si, L - 1) for si, L in zip((2, 3), dlens)]
    cu = np.concatenate([[0], np.cumsum(plens)]).astype(np.int32)
    meta = MI355XAttentionMetadata(
        num_prefills=2, num_prefill_tokens=npf, num_decode_tokens=2, slot_mapping=dev(slots, np.int64), seq_lens=plens + dlens,
        seq_lens_tensor=dev(plens + dlens), max_query_len=max(plens), max_prefill_seq_len=max(plens),
        max_decode_seq_len=max(dlens), query_start_loc=dev(cu), seq_start_loc=dev(cu), context_lens_tensor=dev([0, 0]),
        block_tables=dev(bt), max_context_len=max_context_len)
    impl = MI355XAttentionImpl(Hq, D, scale, Hkv, logits_soft_cap=cap)
    out = impl.forward(*(x.reshape(npf + 2, -1).to(DEV) for x in (q, k, v)), kv_cache, meta).view(-1, Hq, D)
    seqs = [(q[s:e], k[s:e], v[s:e], 0) for s, e in zip(cu[:-1], cu[1:])]
    seqs += [(q[i:i + 1], cat(hk, k[i:i + 1]), cat(hv, v[i:i + 1]), L - 1) for i, L, (hk, hv) in zip((npf, npf + 1), dlens, hist[2:])]
    check(out, refs(seqs, scale, cap), dtype)
