"""More frames than one launch can index (blockIdx.y ends at 65535): S(q) takes them in two batches, F(q, t) cuts the
quantiser's and the rho table's launches and takes the self part in two batches.  The integer sums are exactly additive, so
each long call is compared bit for bit with calls that stay below the limit, and with the host form."""

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import lags
from amof_amd.frames import PackedTrajectory

pytestmark = pytest.mark.gpu

F, NBINS, DQ = 65600, 8, 0.25
HKL = np.array([[1, 0, 0], [0, 1, 1], [1, 1, 2]], dtype=np.int32)      # |q| = 0.628, 0.889, 1.539: bins 2, 3, 6


@pytest.fixture(scope="module")
def long_traj():
    rng = np.random.default_rng(65600)
    pos = np.cumsum(rng.normal(scale=0.05, size=(F, 2, 3)), axis=0) + [[1.0, 2.0, 3.0], [6.0, 5.0, 4.0]]
    return PackedTrajectory(pos, np.eye(3) * 10.0, [30, 7]).to_device(0)


def test_sq_two_batches_equal_two_calls_and_the_host_form(hip_ctx, long_traj):
    import torch
    S = 2
    P = S * (S + 1) // 2

    def fresh():
        return (torch.zeros(NBINS + 1, dtype=torch.int64, device="cuda:0"), torch.zeros(P * NBINS, dtype=torch.int64, device="cuda:0"))

    whole = hip_ctx.sq_accumulate(long_traj, HKL, DQ, NBINS, out=fresh())
    assert hip_ctx.last_path() == "sq" and hip_ctx.last_kernel_launches() == 6         # two batches of three launches
    halves = fresh()
    hip_ctx.sq_accumulate(long_traj, HKL, DQ, NBINS, frame_range=(0, F // 2), out=halves)
    assert hip_ctx.last_kernel_launches() == 3
    _, _, scale, _ = hip_ctx.sq_accumulate(long_traj, HKL, DQ, NBINS, frame_range=(F // 2, F), out=halves)
    assert np.array_equal(scale, whole[2])
    assert torch.equal(halves[0], whole[0]) and torch.equal(halves[1], whole[1])
    counts = whole[0].cpu().numpy()
    assert list(counts[:NBINS]) == [0, 0, F, F, 0, 0, F, 0] and counts[NBINS] == 0
    host = hip_ctx.sq_accumulate(long_traj, HKL, DQ, NBINS)
    assert np.array_equal(host[0], counts[:NBINS].view(np.uint64)) and host[2] == 0
    sums = np.ldexp(whole[1].cpu().numpy().astype(np.float64).reshape(P, NBINS), -whole[2].astype(np.int64)[:, None])
    assert np.array_equal(sums.view(np.uint64), host[1].view(np.uint64)) and np.abs(host[1]).sum() > 0


def test_isf_sliced_launches_and_two_self_batches_equal_split_calls_and_the_host_form(hip_ctx, long_traj):
    import torch
    S, windows = 2, [1]
    lay = _hip.isf_layout(S, 1, NBINS, True)
    total = lags.total_work(F, windows, 1)
    assert total > 65535                    # origins, and one more touched frame: sliced launches, two self batches

    def call(out, work_range):
        return hip_ctx.isf_accumulate(long_traj, HKL, windows, DQ, NBINS, work_range=work_range, out=out)

    whole, scale, _ = call(torch.zeros(lay["size"], dtype=torch.int64, device="cuda:0"), (0, total))
    assert hip_ctx.last_path() == "isf" and hip_ctx.last_kernel_launches() == 3         # the rho table in two launches, one correlation
    halves = torch.zeros(lay["size"], dtype=torch.int64, device="cuda:0")
    call(halves, (0, total // 2))
    assert hip_ctx.last_kernel_launches() == 2
    _, scale_b, _ = call(halves, (total // 2, total))
    assert np.array_equal(scale, scale_b) and torch.equal(halves, whole)
    a = whole.cpu().numpy()
    assert list(a[:NBINS]) == [0, 0, total, total, 0, 0, total, 0] and a[lay["beyond"]] == 0
    counts, coh, selfs, beyond, _ = hip_ctx.isf_accumulate(long_traj, HKL, windows, DQ, NBINS)
    assert np.array_equal(counts.ravel(), a[:NBINS].view(np.uint64)) and beyond[0] == 0
    e = np.zeros((S, S), dtype=np.int64)
    e[np.triu_indices(S)] = scale
    e = e + np.triu(e, 1).T                 # the pair's exponent on both sides
    got_coh = np.ldexp(a[lay["coh"]:lay["self"]].astype(np.float64).reshape(S, S, 1, NBINS), -e[:, :, None, None])
    got_self = np.ldexp(a[lay["self"]:].astype(np.float64).reshape(S, 1, NBINS), -np.diag(e)[:, None, None])
    assert np.array_equal(got_coh.view(np.uint64), coh.view(np.uint64)) and np.abs(coh).sum() > 0
    assert np.array_equal(got_self.view(np.uint64), selfs.view(np.uint64)) and np.abs(selfs).sum() > 0
