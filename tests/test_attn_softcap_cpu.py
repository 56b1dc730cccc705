"""Attention logit soft cap without a GPU: the backend keeps the cap; the C entry points refuse bad arguments before any device call."""
import ctypes

import pytest


def test_backend_keeps_logits_soft_cap():
    from aphrodite_engine_amd.attention import MI355XAttentionImpl
    assert MI355XAttentionImpl(8, 256, 0.0625, 4, logits_soft_cap=50.0).logits_soft_cap == 50.0
    assert MI355XAttentionImpl(8, 256, 0.0625, 4).logits_soft_cap == 0.0
    with pytest.raises(ValueError):
        MI355XAttentionImpl(8, 256, 0.0625, 4, blocksparse_params={}, logits_soft_cap=50.0)      # still refused


@pytest.mark.parametrize("dtype,hd,needle", [("F32", 128, b"dtype"), ("F16", 96, b"128")])
def test_softcap_entry_points_refuse_bad_arguments_before_touching_a_device(dtype, hd, needle):
    from aphrodite_engine_amd import _lib
    L, dt, p = _lib.lib(), getattr(_lib, dtype), ctypes.c_void_p(256)
    calls = [lambda: L.aphro_paged_attention_softcap(p, None, None, None, p, p, p, 1, 4, 2, hd, 0.1, p, p, 1, 16, 16, None, 4 * hd,
                                                     32 * hd, 16 * hd, dt, _lib.KV_AUTO, 1.0, 1.0, 0, 50.0, None),
             lambda: L.aphro_flash_attn_varlen_softcap(p, p, p, p, p, 1, 16, 4, 2, hd, 4 * hd, 2 * hd, 2 * hd, 0.1, 1, None, 0, 50.0, dt, None),
             lambda: L.aphro_context_attention_gathered_softcap(p, p, p, p, p, p, p, p, p, p, 1, 16, 32, 32, 2, 4, 2, hd, 16, 8, 4 * hd, 2 * hd,
                                                                2 * hd, 4 * hd, 0.07, 1.0, 1.0, None, 0, 50.0, dt, _lib.KV_AUTO, p, 1 << 20, None)]
    for call in calls:
        assert call() != 0 and needle in L.aphro_last_error()
