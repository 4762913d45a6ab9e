"""Worker of tests/test_warp_gpu.py: ops.warp_sample through the DEBUG library (FSN_LIB_PATH -> libfsnerf_hip_dbg.so:
warp.hip range-checks every tap offset against the images' extent and notes a source view outside [-1, n_views), -1
being the documented "no source view") - first a case's own rows, forward and backward (its deliberately invalid rows
among them, src_view = -1 too; the row with src_view = n_views is left out: a view past the end is the second pass's
subject), then the forward of the same rows with two rows of src_view = n_views + 5 appended: they must be recorded,
come out as zeros and change no other row - and prints the records as JSON."""
import numpy as np
import torch

import debug_lib as D


def main():
    D.open_debug_library()
    from fs_nerf_amd import ops
    import warp_ref as R
    dev = torch.device("cuda:0")
    out = {}
    for shape in (R.CASES[4], R.CASES[5]):  # 24 x 32 RGBA with per-view K; the smallest cell
        case = R.make_case(*shape, seed=11)
        keep = np.array([k != "s=V" for k in case["kind"]])  # (a view outside [-1, V): the second pass's subject)
        o, d, t, s, poses, images, K = R.case_tensors(case, dev)
        o, d, t, s = (x[torch.as_tensor(keep).to(dev)].contiguous() for x in (o, d, t, s))
        assert int((s == -1).sum()) == 1
        kw = dict(white_bkgd=case["white_bkgd"], border=case["border"], want_uvz=True)
        t.requires_grad_()
        good = ops.warp_sample(o, d, t, s, poses, images, K, **kw)
        good[0].sum().backward()
        torch.cuda.synchronize()
        valid = D.take("warp")
        n_views = poses.shape[0]
        pad = lambda x, row: torch.cat([x.detach(), row.to(dev).expand(2, *x.shape[1:])])
        got = ops.warp_sample(pad(o, torch.ones(1, 3)), pad(d, torch.ones(1, 3)), pad(t, torch.ones(1)),
                              pad(s, torch.tensor([n_views + 5])), poses, images, K, **kw)
        torch.cuda.synchronize()
        rec = D.take("warp")
        n = t.numel()
        zero = all(not bool(x[n:].any()) for x in got)
        equal = all(bool(torch.equal(a[:n].view(torch.uint8), b.view(torch.uint8))) for a, b in zip(got, good))
        if not out:
            out = {"valid": valid, "bad": rec, "n_views": n_views, "first_bad": n_views + 5, "bad_rows_zero": zero,
                   "good_rows_equal": equal}
        else:  # the smallest images must say the same
            assert valid == out["valid"] and rec[0] == out["bad"][0] and rec[2:] == out["bad"][2:], (valid, rec)
            out["bad_rows_zero"] = out["bad_rows_zero"] and zero
            out["good_rows_equal"] = out["good_rows_equal"] and equal
    out["all"] = D.take_all()
    D.emit(out)


if __name__ == "__main__":
    main()
