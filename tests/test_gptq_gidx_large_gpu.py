"""The prompt-sized checkpoint-order GPTQ GEMM (csrc/gptq_gidx_gemm_large.hip: rows in checkpoint order, groups through
g_idx, scales / zeros of the UNSHARDED matrix, M > 64) against the fp64 oracle, through every entry that reaches it:
ops.gptq_gemm_gidx_large, ops.gptq_gemm's routing, HIP-graph replay, the C++ registration, the layer.
The kernel's tile is 256 rows x 128 columns x 32 k, 4 pipeline stages; K is cut into slices of >= 256 k on small grids."""
import functools

import numpy as np
import pytest
import torch

from oracle import quant as oq

pytestmark = pytest.mark.gpu
DEV = "cuda"
#        K_full  gs   k0    K     N
CASES = {"a": (512, 128, 0, 512, 128),        # unsharded; two K slices
         "b": (768, 128, 256, 256, 128),      # shard; G = 6 does not divide K; ONE K slice: the 16-bit epilogue, 8 K tiles
         "c": (7168, 32, 1024, 1024, 256),    # G = 224 table (84 KiB); two column tiles; four K slices
         "d": (2048, 64, 512, 1536, 128),     # split-K: six slices of 8 K tiles
         "e": (64, 32, 0, 64, 128)}           # two K tiles: shorter than the pipeline
TOL = {torch.float16: 3e-3, torch.bfloat16: 1.6e-2}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from aphrodite_engine_amd import _custom_ops, _lib
    _lib.lib()
    return _custom_ops


@functools.lru_cache(maxsize=None)
def _weights(name, n, gmap):
    k_full, gs, k0, k, n_case = CASES[name]
    n = n or n_case
    rng = np.random.default_rng(ord(name) + n)
    w = (rng.standard_normal((k_full, n)) * 0.02).astype(np.float16)
    _, q, s, zp = oq.quantize_weights(w, 4, gs, zero_points=True)
    perm = rng.permutation(k_full)
    g_idx = (np.arange(k_full) // gs)[perm][k0:k0 + k]
    if gmap == "sequential":
        g_idx = (k0 + np.arange(k)) // gs
    elif gmap == "constant":
        g_idx = np.full(k, k_full // gs - 1)
    return oq.gptq_pack(q[perm][k0:k0 + k]), oq.gptq_pack_zeros(zp), s.astype(np.float32), g_idx.astype(np.int32)


def case(name, m, dtype, n=None, gmap="perm"):
    """-> (device arguments (a, qweight, qzeros, scales, g_idx), fp64 oracle result on the rounded a / scales)."""
    qw, qz, s, g_idx = _weights(name, n, gmap)
    rng = np.random.default_rng(m)
    a = torch.from_numpy(rng.standard_normal((m, qw.shape[0] * 8)).astype(np.float32)).to(DEV).to(dtype)
    s_t = torch.from_numpy(s).to(DEV).to(dtype)
    ref = oq.gptq_gemm(a.float().cpu().numpy(), qw, qz, s_t.float().cpu().numpy(), g_idx, False)
    return (a, torch.from_numpy(qw).to(DEV), torch.from_numpy(qz).to(DEV), s_t, torch.from_numpy(g_idx).to(DEV)), ref


def close(out, ref, dtype):
    got = out.float().cpu().numpy()
    assert got.shape == ref.shape and np.abs(got - ref).mean() / np.abs(ref).mean() < 0.04
    np.testing.assert_allclose(got, ref, rtol=TOL[dtype], atol=TOL[dtype] * np.abs(ref).max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m", [65, 129, 257])            # partial last M tile; idle second row of waves; two M tiles
@pytest.mark.parametrize("name", list(CASES))
def test_gidx_large_parity(ops, name, m, dtype):
    from aphrodite_engine_amd import _lib
    args, ref = case(name, m, dtype)
    k, n, groups = args[0].shape[1], args[1].shape[1], args[3].shape[0]
    assert ops.gptq_gidx_large_ok(m, n, k, groups, dtype)
    split = _lib.lib().aphro_gptq_gemm_gidx_large_workspace_bytes(m, n, k, groups, _lib.F16)
    assert (split == 6 * m * n * 4) if name == "d" else (split == 0) == (name in "be")
    close(ops.gptq_gemm_gidx_large(*args), ref, dtype)


@pytest.mark.parametrize("gmap", ["sequential", "constant"])
def test_gidx_large_degenerate_group_maps(ops, gmap):
    args, ref = case("b", 65, torch.float16, gmap=gmap)
    close(ops.gptq_gemm_gidx_large(*args), ref, torch.float16)


@pytest.mark.parametrize("m", [64, 65, 129])
def test_gidx_large_routing(ops, m):
    args, ref = case("c", m, torch.float16)
    out = ops.gptq_gemm(*args, False, 4)
    close(out, ref, torch.float16)
    assert torch.equal(out, (ops.gptq_gemm_gidx if m == 64 else ops.gptq_gemm_gidx_large)(*args))
    if m == 65:
        assert not ops.gptq_gidx_large_ok(m, 72, 256, 6, torch.float16)
        assert not ops.gptq_gidx_large_ok(m, 128, 256, 233, torch.float16)      # the table of 233 groups does not fit the LDS
        args72, ref72 = case("b", m, torch.float16, n=72)        # no 128-column tiling: the reconstruct + library GEMM path
        close(ops.gptq_gemm(*args72, False, 4), ref72, torch.float16)


def test_gidx_large_graph_replay(ops):
    """Split-K through slabs + a reduce launch: nothing to reset, so every replay equals the eager call bit for bit."""
    args, _ = case("d", 65, torch.float16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gptq_gemm_gidx_large(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.gptq_gemm_gidx_large(*args)
    for seed in range(3):
        args[0].copy_(torch.randn(args[0].shape, generator=torch.Generator().manual_seed(seed)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.gptq_gemm_gidx_large(*args))


def test_gidx_large_cpp_op(ops):
    from aphrodite_engine_amd import torch_cpp
    torch_cpp.load()
    args, _ = case("b", 129, torch.float16)
    got = getattr(torch.ops, torch_cpp.NAMESPACE).gptq_gemm(*args, False, 4)
    assert torch.equal(got, ops.gptq_gemm(*args, False, 4)) and torch.equal(got, ops.gptq_gemm_gidx_large(*args))


def test_gidx_large_layer(ops):
    """desc_act + row-parallel: the layer stays in checkpoint order (ExllamaState.UNUSED); a prompt reaches the kernel."""
    import torch.nn as nn
    from aphrodite_engine_amd.quantization.gptq import ExllamaState, GPTQConfig
    k_full, gs, _, k, n = CASES["b"]
    (a, qw, qz, s, g_idx), ref = case("b", 129, torch.float16)
    method = GPTQConfig(4, gs, True).get_quant_method(nn.Linear(1, 1), "")
    layer = nn.Module()
    method.create_weights(layer, k, [n], k_full, n, torch.float16, weight_loader=None)
    layer.to(DEV)
    for name, val in (("qweight", qw), ("qzeros", qz), ("scales", s), ("g_idx", g_idx)):
        getattr(layer, name).data.copy_(val)
    method.process_weights_after_loading(layer)
    assert layer.exllama_state == ExllamaState.UNUSED
    close(method.apply(layer, a), ref, torch.float16)
