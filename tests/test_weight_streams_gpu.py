"""GPU: the one device packer (csrc/mlp.hip, k_pack_stream) writes, byte for byte, what the host packer writes - the
same piece function (csrc/mlp_pack.hpp pack_piece) compiled for both - for all three weight streams: the forward blob
(header and aux region included), the dgrad chain's transposed stream, the input gradient's weight slices.  The host
side is pinned on the CPU (test_pack_layout.py, test_weight_streams_cpu.py); this ties the device side to it.
Networks: the corners of tests/wstream_ref.py and 6 x 128 with skips (1, 3)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_weight_streams_cpu import BWD, FLAGS, IG, NETS, TRAIN_PRECS, make_desc, make_weights, ptrs, stream_bytes

pytestmark = pytest.mark.gpu
INFER_PRECS = [0, 1, 2, 3, 4, 6]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=list(NETS))
def net(request, dev):
    """(name, descriptor, host weights and biases, their device copies), made once per network."""
    n = NETS[request.param]
    ws = make_weights(n)
    rng = np.random.default_rng(3)
    bs = [rng.standard_normal(w.shape[0]).astype(np.float32) for w in ws]
    dws, dbs = [torch.from_numpy(w).to(dev) for w in ws], [torch.from_numpy(b).to(dev) for b in bs]
    return request.param, n, make_desc(n), ws, bs, dws, dbs


def test_forward_blob_device_equals_host(net, dev):
    from fs_nerf_amd import _lib as L
    from fs_nerf_amd import ops
    name, n, desc, ws, bs, dws, dbs = net
    n_gemm = n[0] + 2
    cases = [(p, None) for p in INFER_PRECS] + [(L.FSN_PREC_FP16X3U, [(-1) ** g * (g % 5 + 1) for g in range(n_gemm)])]
    for prec, exps in cases:
        nb = L.lib().fsn_mlp_blob_bytes(C.byref(desc), prec)
        host = np.full(nb, 0xAB, dtype=np.uint8)
        ex = None if exps is None else (C.c_int32 * n_gemm)(*exps)
        L.check(L.lib().fsn_mlp_pack_scaled_host(C.byref(desc), prec, ptrs(ws), ptrs(bs), ex, host.ctypes.data), "host pack")
        got = ops.PackedMLP(desc, prec, dev)
        got.blob.zero_()  # (the host packer zeroes the alignment gap in front of the stream, the device packer skips it)
        got.pack(dws, dbs, exps)
        assert got.blob.numel() == nb and np.array_equal(got.blob.cpu().numpy(), host), (name, prec, exps)


def test_training_streams_device_equal_host(net, dev):
    from fs_nerf_amd import _lib as L
    from fs_nerf_amd import ops
    name, n, desc, ws, bs, dws, dbs = net
    for prec in TRAIN_PRECS:
        for kind, wx, wd in [(BWD, 0, 0)] + [(IG, x, d) for x, d in FLAGS]:
            nb = stream_bytes(desc, prec, kind, wx, wd)
            host = np.full(nb, 0xAB, dtype=np.uint8)
            L.check(L.lib().fsn_weight_stream_pack_host(C.byref(desc), prec, kind, wx, wd, ptrs(ws), host.ctypes.data),
                    "fsn_weight_stream_pack_host")
            got = torch.full((nb + 256,), 0xAB, dtype=torch.uint8, device=dev)  # a guard behind the stream
            ops._launch("fsn_weight_stream_pack", dev, C.byref(desc), prec, kind, wx, wd, ops._ptr_array(dws), got)
            out = got.cpu().numpy()
            assert np.array_equal(out[:nb], host) and (out[nb:] == 0xAB).all(), (name, prec, kind, wx, wd)
