"""One index, one workspace, every pipeline in turn (hdb_ws.h, hdb_api.hip).

Every top-k pipeline lays its own regions out in the index's single scratch buffer.  Index A serves a sequence of calls that walks
through all four layouts -- the 1-4-query shadow behind the 5-bit plane, the shadow batch, the single launch, the multi-kernel
pipeline (bit metrics, manhattan, the exact path) and the full sort of k > 2048 -- and then the first calls again.  Each call must
return the indices, score bits and status words of the same call on a fresh index B that has served nothing else, and the
workspace of A never shrinks.

20 000 rows at d = 128 is the smallest shape that sits above the candidate cap, has a matrix-core geometry and is a width the int8
batch kernel accepts."""
import numpy as np
import pytest

from hyperdb import _native

pytestmark = pytest.mark.gpu

M = _native.METRIC_IDS
N, D = 20000, 128

# (label, options for the call, queries, k, metric, expected stats)
CALLS = [
    ("1 cosine query, shadow + plane", {}, 1, 100, "cosine_similarity", {"quant": 1, "plane": 1}),
    ("8 dot queries, shadow batch", {}, 8, 100, "dot_product", {"quant": 1}),
    # (d = 128 has no one-kernel top-k of 1-4 queries: the call takes the batched single launch, stat fused = 2)
    ("1 query, single launch", {"use_quant": 0}, 1, 100, "cosine_similarity", {"quant": 0, "fused": 2, "path": 1}),
    ("64 pearson queries", {}, 64, 100, "pearson_correlation", {}),
    ("2 hamming queries", {}, 2, 100, "hamming_distance", {}),
    ("3 manhattan queries", {}, 3, 100, "manhattan_distance", {}),
    ("5 queries, force_exact", {"force_exact": 1}, 5, 100, "cosine_similarity", {"path": 2}),
    ("2 pearson queries, k = 2049", {}, 2, 2049, "pearson_correlation", {"path": 3}),
]
SEQUENCE = list(range(len(CALLS))) + [0, 1, 2]        # ... then calls 1 to 3 again
DEFAULTS = {"use_quant": 1, "force_exact": 0}


@pytest.fixture(scope="module")
def data():
    import torch
    g = torch.Generator(device="cuda").manual_seed(20)
    V = torch.randn((N, D), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
    Q = torch.randn((64, D), generator=g, device="cuda", dtype=torch.float32)
    return V, Q


def _index(V):
    ix = _native.GpuIndex(V)
    for name in ("quant_min_n", "quant_batch_min_n", "plane_min_n"):
        ix.set_option(name, 0)
    return ix


def _call(ix, Q, call):
    label, opts, nq, k, metric, want = call
    for name, v in opts.items():
        ix.set_option(name, v)
    try:
        idx, sc, st = ix.topk_device(Q[:nq].contiguous(), k, M[metric])
        out = (idx.cpu().numpy(), sc.cpu().numpy().view(np.int32), st.cpu().numpy())
        for name, v in want.items():
            assert ix.stat(name) == v, f"{label}: stat {name} = {ix.stat(name)}, expected {v}"
    finally:
        for name in opts:
            ix.set_option(name, DEFAULTS[name])
    return out


def test_every_pipeline_on_one_workspace(data):
    V, Q = data
    fresh = []                                   # each call alone on an index that has served nothing else
    for call in CALLS:
        B = _index(V)
        try:
            fresh.append(_call(B, Q, call))
        finally:
            B.close()
    A = _index(V)
    try:
        ws = A.stat("ws_bytes")
        for step, c in enumerate(SEQUENCE):
            got = _call(A, Q, CALLS[c])
            for what, a, b in zip(("indices", "score bits", "status"), got, fresh[c]):
                assert np.array_equal(a, b), f"step {step} ({CALLS[c][0]}): {what} differ from the fresh index"
            assert A.stat("ws_bytes") >= ws, f"step {step} ({CALLS[c][0]}): the workspace shrank from {ws} to {A.stat('ws_bytes')}"
            ws = A.stat("ws_bytes")
    finally:
        A.close()


def test_shadow_workspace_does_not_depend_on_k(data):
    V, Q = data
    ix = _index(V)
    try:
        sizes = []
        for k in (1, 100, 128):
            ix.topk_device(Q[:1].contiguous(), k, M["cosine_similarity"])
            assert ix.stat("quant") == 1, f"k = {k}: the call did not take the shadow"
            sizes.append(ix.stat("ws_bytes"))
        assert sizes[0] > 0 and sizes[0] == sizes[1] == sizes[2], f"ws_bytes over k = 1, 100, 128: {sizes}"
    finally:
        ix.close()
