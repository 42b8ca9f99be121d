"""CPU checks of the full-catalogue ranking / top-K boundary (no GPU): the header declares the new calls, the ctypes
table binds them, and ops.full_topk rejects a bad k before anything touches a device."""
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "recsys_hip.h")
NEW = ["rs_full_rank", "rs_full_topk", "rs_full_ws_bytes", "rs_rank_to_metrics"]


def declared_symbols():
    return set(re.findall(r"^(?:int|int64_t) (rs_\w+)\(", open(HEADER).read(), flags=re.M))


def test_header_declares_the_full_rank_calls():
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
    text = open(HEADER).read()
    m = re.search(r"^#define RS_TOPK_MAX (\d+)$", text, flags=re.M)
    assert m and int(m.group(1)) == 128


def test_signatures_bind_the_full_rank_calls():
    import rbm_amd._lib as L
    from rbm_amd import ops
    for s in NEW:
        assert s in L.SIGNATURES, s
    assert L.RESTYPES["rs_full_ws_bytes"] is L.C.c_int64
    assert len(L.SIGNATURES["rs_full_topk"]) == len(L.SIGNATURES["rs_full_rank"])    # target / ts out <-> K / scores
    assert ops.RS_TOPK_MAX == 128


def test_ws_bytes_is_host_only_and_far_below_a_score_matrix():
    """Sizing needs no device; at B = 64 over 1M items with K = 10 the workspace is a few MB, not B x V x 4."""
    import rbm_amd._lib as L
    lib = L.lib()
    B, V = 64, 1_000_000
    rank_only = lib.rs_full_ws_bytes(L.BF16, B, 64, V, 0)
    topk = lib.rs_full_ws_bytes(L.BF16, B, 64, V, 10)
    assert 0 < rank_only <= 4096
    assert rank_only < topk < B * V * 4 // 8 // 2
    assert lib.rs_full_ws_bytes(L.BF16, B, 64, V, 129) == 0


@pytest.mark.parametrize("k", [0, 129, -1])
def test_full_topk_rejects_k_before_any_device_call(k):
    import torch

    from rbm_amd import ops
    h = torch.zeros(2, 8)            # CPU tensors: a device call would fail differently
    E = torch.zeros(5, 8)
    with pytest.raises(ValueError):
        ops.full_topk(h, E, k)
