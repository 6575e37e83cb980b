"""NDB / JSD and the k-means bin pass on the device (fd_bins_pass, fastdiff_amd.diversity, TrainCorpus.fit_bins, infer --ndb_bins) against
the oracle tests/diversity_ref.py: the header's standardisation in float32, then float64 distances, Lloyd's iteration and the statistics.

Bars.  None is tuned on the device.
  * assignment: with d64 the float64 squared distance over the float32 z, d64(assigned) - min_k d64(k) <= tau = 2 g (E_assigned + E_best),
    E_k = ||c_k||^2 / 2 + sum_d |z_d| |c_kd|, g = n u / (1 - n u), n = D + 2, u = 2^-24: the rounding bound of s_k = h_k - dot_k (h: D
    fmas and a halving, dot: D fmas, one subtraction).  Nothing on top.  The CPU test shows that numpy's restatement of the header's
    float32 form keeps it on the same inputs.
  * record: counts = the bincount of the returned assignments, moved exact; inertia within 1e-12 relative of the float64 sum over the
    device's own assignments.
  * update: |centroids_out - float64 mean| <= FD_BINS_CHUNK u mean|z_d| over the bin (a float32 sum of at most FD_BINS_CHUNK terms per
    chunk) + u |mean| (the quotient's rounding); an empty bin keeps its centroid bit for bit.
  * determinism: bits.
Shapes: N at the borders of the 32-row matrix tile, of the 128-row block and of FD_BINS_CHUNK; D and K at the borders of the 32-wide tiles.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import fastdiff_amd
from fastdiff_amd import _capi, _wave, diversity as dv
import diversity_ref as ref

gpu = pytest.mark.gpu
C = dv.CHUNK
# (N, D, K, ld, floats the first row lies behind a 16-byte boundary)
SHAPES = [(1, 4, 1, 4, 0), (31, 36, 2, 36, 0), (32, 80, 31, 80, 0), (33, 128, 32, 128, 1), (257, 80, 33, 96, 0), (C - 1, 4, 50, 4, 1),
          (C, 36, 128, 36, 0), (C + 1, 80, 50, 96, 1), (2 * C + 1, 128, 128, 128, 0), (2 * C + 1, 80, 50, 80, 0)]
IDS = ["N%d-D%d-K%d-ld%d-off%d" % s for s in SHAPES]


@functools.lru_cache(maxsize=None)
def inputs(N, D, K):
    """x, shift, scale, centroids (the last bin far away, so empty, when K >= 3), the previous assignments, z; shared, never changed."""
    x, shift, scale, cent = ref.gaussians(100 + N + D + K, N, D, K, spread=0.5)
    if K >= 3:
        cent[K - 1] = 100.0
    prev = np.random.default_rng(N).integers(-1, K, N).astype(np.int32)
    z = ref.standardise(x, shift, scale)
    for a in (x, shift, scale, cent, prev, z):
        a.setflags(write=False)
    return x, shift, scale, cent, prev, z


# ------------------------------------------------------------------------------------------------------------------ CPU
@functools.lru_cache(maxsize=None)
def near_ties(N=513, D=80, K=33):
    """The inputs of (N, D, K) with bins 1, 2 and 32 moved to within 1e-6 of bin 0, 3 and 31: their rows sit on near ties, where the
    float32 score decides differently from float64 and the bound is what holds."""
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    rng = np.random.default_rng(77)
    cent = cent.copy()
    for new, old in ((1, 0), (2, 3), (32, 31)):
        cent[new] = cent[old] + (1e-6 * rng.normal(size=D)).astype(np.float32)
    cent.setflags(write=False)
    return x, shift, scale, cent, prev, z


def test_the_float32_form_keeps_the_bound_on_near_ties_where_it_differs_from_float64():
    x, shift, scale, cent, prev, z = near_ties()
    a = ref.assign32(z, cent)
    tau, excess = ref.tau(z, cent, a)
    print(f"largest excess / tau of the float32 form: {float((excess / tau).max()):.3g}; rows that differ from float64's: {int((a != ref.assign64(z, cent)).sum())}")
    assert (excess <= tau).all() and (a != ref.assign64(z, cent)).any()


def test_the_module_is_exported_and_mirrors_the_header():
    assert "diversity" in fastdiff_amd.__all__ and fastdiff_amd.diversity is dv and callable(fastdiff_amd.TrainCorpus.fit_bins)
    lib = _capi.load()
    assert lib.fd_bins_chunk() == dv.CHUNK == 4096 and lib.fd_bins_record_bytes() == dv.RECORD.itemsize == 1056
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    assert "#define FD_BINS_CHUNK 4096" in header and "/* 1056 bytes */" in header


def test_ndb_jsd_against_the_restatement():
    rng = np.random.default_rng(5)
    for K in (1, 2, 50, 128):
        for _ in range(5):
            r, q = rng.integers(0, 1000, K), rng.integers(0, 50, K)
            r[0] += 1
            q[0] += 1
            if K > 2:
                r[1] = q[1] = 0
            for alpha in (0.05, 0.01):
                got, want = dv.ndb_jsd(r, q, alpha), ref.ndb_jsd(r, q, alpha)
                assert got["ndb"] == want["ndb"] and abs(got["ndb_over_k"] - want["ndb_over_k"]) <= 1e-12
                assert abs(got["jsd"] - want["jsd"]) <= 1e-12 and np.abs(got["z"] - want["z"]).max() <= 1e-12 * max(1.0, np.abs(want["z"]).max())
                assert (got["different"] == want["different"]).all() and got["n"] == q.sum() and (got["counts"] == q).all()


def test_ndb_jsd_on_equal_disjoint_and_empty_bins():
    r = np.array([10, 0, 300, 7, 0, 55])
    same = dv.ndb_jsd(r, 3 * r)
    assert same["ndb"] == 0 and same["jsd"] == 0.0 and not same["different"].any()
    a, b = np.array([40, 0, 25, 0, 0, 0]), np.array([0, 30, 0, 0, 90, 0])
    apart = dv.ndb_jsd(a, b)
    assert abs(apart["jsd"] - np.log(2.0)) <= 1e-15
    assert (apart["different"] == ((a + b) > 0)).all() and apart["ndb"] == 4 and apart["ndb_over_k"] == 4 / 6
    assert not apart["different"][3] and not apart["different"][5] and apart["z"][3] == 0.0          # empty in both: not different
    for bad in ((r, r[:3]), (r, -r), (r, 0 * r), (0 * r, r)):
        with pytest.raises(ValueError):
            dv.ndb_jsd(*bad)
    with pytest.raises(ValueError):
        dv.ndb_jsd(r, r, alpha=1.0)


def test_the_c_call_refuses_by_name_before_it_looks_at_the_handle():
    lib = _capi.load()
    ok = dict(x=64, N=10, D=8, ld=8, shift=None, scale=None, cent=1 << 20, K=3, assign=None, out=2 << 20, rec=3 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.fd_bins_pass(None, a["x"], a["N"], a["D"], a["ld"], a["shift"], a["scale"], a["cent"], a["K"], a["assign"], a["out"], a["rec"], None)
        return rc, (lib.fd_last_error(None) or b"").decode()

    for kw, word in ((dict(x=None), "null x"), (dict(cent=None), "null centroids"), (dict(N=0), "N = 0"), (dict(N=(1 << 40) + 1), "N = "),
                     (dict(D=0), "D = 0"), (dict(D=6), "D = 6"), (dict(D=132, ld=132), "D = 132"), (dict(K=0), "K = 0"), (dict(K=129), "K = 129"),
                     (dict(ld=7), "ld = 7"), (dict(x=66), "aligned"), (dict(shift=128), "scale is null"), (dict(scale=128), "shift is null"),
                     (dict(out=None, rec=None), "nothing to write"), (dict(out=(1 << 20) + 4), "overlaps"), (dict(out=(1 << 20) - 4 * 23), "overlaps")):
        rc, msg = call(**kw)
        assert rc == _capi.FD_ERR_INVALID and msg.startswith("fd_bins_pass: ") and word in msg, (kw, rc, msg)
    rc, msg = call()
    assert rc == _capi.FD_ERR_INVALID and "null handle" in msg          # everything else in order: only the handle is missing
    rc, msg = call(out=(1 << 20) + 4 * 24)
    assert "null handle" in msg                                          # (behind the centroids' last element: no overlap)


def test_fit_and_bins_pass_refuse_wrong_arguments():
    x = torch.zeros(10, 8)
    for bad, kw in ((np.zeros((10, 8), np.float32), {}), (x.double(), {}), (x[:, :4], {}), (torch.zeros(10, 6), {}), (torch.zeros(10, 132), {}),
                    (torch.zeros(0, 8), {}), (x, dict(K=0)), (x, dict(K=129)), (x, dict(K=11)), (x, dict(K=2, iters=0)), (x, dict(K=2, n_init=0)),
                    (x, dict(K=2, check_every=0)), (x, dict(K=2, ld=16)), (x, dict(K=2))):          # the last: everything in order but the device
        with pytest.raises(ValueError):
            dv.fit(bad, **kw)
    c = torch.zeros(3, 8)
    for kw in (dict(centroids=torch.zeros(3, 4)), dict(centroids=torch.zeros(129, 8)), dict(shift=torch.zeros(8)), dict(shift=torch.zeros(8), scale=torch.zeros(4)),
               dict(assign=torch.zeros(10, dtype=torch.int64)), dict(assign=torch.zeros(9, dtype=torch.int32)), dict(record=False), {}):
        with pytest.raises(ValueError):
            dv.bins_pass(x, **dict(dict(centroids=c), **kw))
    with pytest.raises(ValueError):
        dv.frames(torch.zeros(2, 80, 5))


def test_bins_save_and_load_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    b = dv.Bins(rng.normal(size=(5, 8)), rng.normal(size=8), rng.uniform(0.5, 2.0, 8), rng.integers(0, 99, 5), 12.5, 7)
    assert (b.K, b.D) == (5, 8) and b.centroids.dtype == np.float32 and b.ref_counts.dtype == np.int64
    b.save(tmp_path / "bins.npz")
    c = dv.Bins.load(tmp_path / "bins.npz")
    for name in ("centroids", "shift", "scale", "ref_counts"):
        assert getattr(b, name).tobytes() == getattr(c, name).tobytes() and getattr(b, name).dtype == getattr(c, name).dtype, name
    assert (c.inertia, c.passes, c.K, c.D) == (12.5, 7, 5, 8)


def _stub_pass(calls):
    """fd_bins_pass on host tensors by the oracle (float64 distances), for the loop of fit."""
    def fn(lib, handle, stream, x, N, D, ld, shift, scale, centroids, assign, out, rec):
        z = ref.standardise(x.numpy(), shift.numpy(), scale.numpy())
        r = ref.lloyd_pass(z, centroids.numpy(), assign.numpy())
        assign.copy_(torch.from_numpy(r["assign"].astype(np.int32)))
        out.copy_(torch.from_numpy(r["centroids"].astype(np.float32)))
        raw = np.zeros(1, dv.RECORD)
        raw["counts"][0, : centroids.shape[0]] = r["counts"]
        for k in ("inertia", "moved", "nonfinite", "empty"):
            raw[k] = r[k]
        rec.copy_(torch.from_numpy(raw.view(np.uint8).reshape(-1)))
        calls.append(r["moved"])
    return fn


def test_the_loop_of_fit_on_a_stubbed_device_call(monkeypatch):
    """Restarts, the stop at moved == 0 seen only every check_every passes, the lowest inertia, self-consistent counts."""
    calls = []
    monkeypatch.setattr(dv, "_pass", _stub_pass(calls))
    monkeypatch.setattr(dv, "_need_device", lambda x, who: None)
    monkeypatch.setattr(_wave, "default_handle", lambda t: (None, None, None))
    xn, _ = ref.blobs(3, 301, 8, 3, sep=12.0)
    x = torch.from_numpy(xn)
    fits = {}
    for ce in (1, 4):
        del calls[:]
        b = dv.fit(x, K=3, iters=20, n_init=3, seed=1, check_every=ce)
        per = [i + 1 for i, m in enumerate(calls) if m == 0]          # the pass of each restart that moved nothing
        assert len(per) >= 3 and len(calls) % ce == 0
        fits[ce] = b
        z = ref.standardise(xn, b.shift, b.scale)
        r = ref.lloyd_pass(z, b.centroids)
        assert (r["counts"] == b.ref_counts).all() and abs(r["inertia"] - b.inertia) <= 1e-12 * b.inertia and b.ref_counts.sum() == 301
    assert fits[1].centroids.tobytes() == fits[4].centroids.tobytes() and fits[1].passes == fits[4].passes          # reading the record less often changes nothing
    mean, std = xn.astype(np.float64).mean(0), xn.astype(np.float64).std(0)
    assert np.abs(fits[1].shift - mean).max() <= 1e-6 and np.abs(fits[1].scale - 1 / std).max() <= 1e-6
    inertias = []
    for r in range(3):          # the winner is the restart with the lowest inertia
        del calls[:]
        inertias.append(dv.fit(x, K=3, iters=20, n_init=1, seed=1 + r).inertia)
    assert fits[1].inertia == min(inertias)
    flat = torch.cat([x[:, :4], torch.full((301, 4), 3.0)], 1)
    b = dv.fit(flat, K=2, iters=3, n_init=1)
    assert (b.scale[4:] == 1.0).all() and (b.shift[4:] == 3.0).all()          # zero variance: scale 1
    del calls[:]
    assert dv.fit(x, K=3, iters=1, n_init=1, seed=1).passes == 1 and len(calls) == 1
    rows = dv.initial_rows(301, 3, 1)
    assert torch.equal(rows, torch.randperm(301, generator=torch.Generator().manual_seed(1))[:3]) and len(set(rows.tolist())) == 3


@pytest.mark.parametrize("N, D, K, ld, off", SHAPES, ids=IDS)
def test_the_float32_form_of_the_header_keeps_the_assignment_bound(N, D, K, ld, off):
    """The bar of the device test is one the arithmetic keeps: numpy's restatement of s_k = fl(h_k - dot_k) on the same inputs."""
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    a = ref.assign32(z, cent)
    tau, excess = ref.tau(z, cent, a)
    assert (excess <= tau).all() and (tau > 0).all()
    print(f"largest excess / tau of the float32 form: {float((excess / tau).max()):.3g}; rows that differ from float64's: {int((a != ref.assign64(z, cent)).sum())}")


def fit_blobs():
    return ref.blobs(11, 3001, 80, 5)


@functools.lru_cache(maxsize=None)
def fit_oracle():
    """Lloyd's iteration of the oracle on the blobs from the rows diversity.initial_rows picks: [(centroids in, pass)]."""
    x, _ = fit_blobs()
    cent = x[dv.initial_rows(x.shape[0], 5, 0).numpy()].copy()
    trail, prev = [], np.full(x.shape[0], -1)
    for _ in range(30):
        r = ref.lloyd_pass(x, cent, prev)
        trail.append((cent, r))
        if r["moved"] == 0:
            break
        cent, prev = r["centroids"].astype(np.float32), r["assign"]
    return trail


def test_the_blobs_of_the_whole_fit_leave_no_room_for_a_tie():
    """Equal assignments are demanded of the device on this set: every row's runner-up is further away than twice the rounding bound, in
    every pass of the oracle's run."""
    x, _ = fit_blobs()
    trail = fit_oracle()
    assert 2 <= len(trail) < 30 and trail[-1][1]["moved"] == 0
    for cent, r in trail:
        d = np.sort(ref.dist64(x, cent), axis=1)
        tau, _ = ref.tau(x, cent, r["assign"])
        assert cent.shape[0] == 1 or ((d[:, 1] - d[:, 0]) > 4 * tau).all()


# ------------------------------------------------------------------------------------------------------------------ GPU
def dev_rows(x, ld=None, off=0):
    """The rows x [N, D] in device memory ld floats apart, the first `off` floats behind a 16-byte boundary, in a buffer that ends with the
    last row's D floats; what lies between the rows is NaN."""
    N, D = x.shape
    ld = ld or D
    buf = torch.full((off + (N - 1) * ld + D,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = torch.as_strided(buf, (N, D), (ld, 1), off)
    v.copy_(torch.from_numpy(np.array(x, np.float32)))
    return v


def run_pass(x, cent, shift=None, scale=None, prev=None, ld=None, off=0, update=True):
    """-> dict(assign [N] int64 or None, rec, out [K, D] float32 or None, raw: the bytes of all three)"""
    xd = dev_rows(x, ld, off)
    assign = torch.from_numpy(np.array(prev, np.int32)).cuda() if prev is not None else None
    rec, out = dv.bins_pass(xd, torch.from_numpy(np.array(cent, np.float32)).cuda(), None if shift is None else torch.from_numpy(np.array(shift, np.float32)).cuda(),
                            None if scale is None else torch.from_numpy(np.array(scale, np.float32)).cuda(), assign=assign, update=update,
                            ld=None if (ld or x.shape[1]) == x.shape[1] else ld)
    a = assign.cpu().numpy().astype(np.int64) if assign is not None else None
    o = out.cpu().numpy() if out is not None else None
    raw = (b"" if a is None else a.tobytes()) + (b"" if o is None else o.tobytes()) + rec["counts"].tobytes() + np.float64(rec["inertia"]).tobytes() + \
        np.array([rec["moved"], rec["nonfinite"], rec["empty"], rec["status"]]).tobytes()
    return {"assign": a, "rec": rec, "out": o, "raw": raw}


@functools.lru_cache(maxsize=None)
def device(N, D, K, ld, off):
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    return run_pass(x, cent, shift, scale, prev, ld, off)


@gpu
@pytest.mark.parametrize("N, D, K, ld, off", SHAPES, ids=IDS)
def test_every_row_is_assigned_to_a_nearest_bin_up_to_the_rounding_bound(N, D, K, ld, off):
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    a = device(N, D, K, ld, off)["assign"]
    assert a.shape == (N,) and a.min() >= 0 and a.max() < K
    tau, excess = ref.tau(z, cent, a)
    print(f"largest excess / tau: {float((excess / tau).max()):.3g}; rows that differ from float64's: {int((a != ref.assign64(z, cent)).sum())}")
    assert (excess <= tau).all()


@gpu
def test_near_ties_are_decided_within_the_rounding_bound():
    x, shift, scale, cent, prev, z = near_ties()
    a = run_pass(x, cent, shift, scale, prev)["assign"]
    tau, excess = ref.tau(z, cent, a)
    print(f"largest excess / tau on near ties: {float((excess / tau).max()):.3g}; rows that differ from float64's: {int((a != ref.assign64(z, cent)).sum())}")
    assert (excess <= tau).all()


@gpu
@pytest.mark.parametrize("N, D, K, ld, off", SHAPES, ids=IDS)
def test_the_record_is_exact_on_the_devices_own_assignments(N, D, K, ld, off):
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    got = device(N, D, K, ld, off)
    a, rec = got["assign"], got["rec"]
    counts = np.bincount(a, minlength=K)
    assert (rec["counts"] == counts).all() and rec["counts"].dtype == np.int64
    want = ref.inertia64(z, cent, a)
    print(f"inertia {rec['inertia']!r}, float64 {want!r}")
    assert abs(rec["inertia"] - want) <= 1e-12 * want
    assert rec["moved"] == int((a != prev).sum()) and rec["nonfinite"] == 0 and rec["empty"] == int((counts == 0).sum())
    assert rec["status"] == dv.OK and (K < 3 or rec["empty"] >= 1)


@gpu
@pytest.mark.parametrize("N, D, K, ld, off", SHAPES, ids=IDS)
def test_the_update_is_the_mean_within_the_bound_of_a_chunked_float32_sum(N, D, K, ld, off):
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    got = device(N, D, K, ld, off)
    mean, bound = ref.update_bound(z, got["assign"], cent, C)
    err = np.abs(got["out"].astype(np.float64) - mean)
    filled = got["rec"]["counts"] > 0
    print(f"largest error / bound: {float((err[filled] / bound[filled]).max()):.3g}")
    assert (err[filled] <= bound[filled]).all()
    assert got["out"][~filled].tobytes() == cent[~filled].tobytes()          # an empty bin keeps its centroid bit for bit


@gpu
@pytest.mark.parametrize("N, D, K, ld, off", [SHAPES[0], SHAPES[4], SHAPES[7], SHAPES[8]], ids=[IDS[0], IDS[4], IDS[7], IDS[8]])
def test_two_runs_and_every_layout_give_the_same_bits(N, D, K, ld, off):
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    first = device(N, D, K, ld, off)["raw"]
    assert run_pass(x, cent, shift, scale, prev, ld, off)["raw"] == first                         # again
    assert run_pass(x, cent, shift, scale, prev, ld, 1 - off)["raw"] == first                     # 4 bytes off a 16-byte boundary, or on it
    assert run_pass(x, cent, shift, scale, prev, D if ld != D else D + 16, off)["raw"] == first   # packed rows, or the same rows 16 floats further apart
    assert run_pass(z, cent, None, None, prev, ld, off)["raw"] == first                           # a standardised copy, shift = scale = NULL
    only = run_pass(x, cent, shift, scale, None, ld, off, update=False)                          # assignment only: the same counts, moved = -1
    assert only["rec"]["moved"] == -1 and only["out"] is None and only["rec"]["counts"].tobytes() == device(N, D, K, ld, off)["rec"]["counts"].tobytes()
    assert only["rec"]["inertia"] == device(N, D, K, ld, off)["rec"]["inertia"]


@gpu
def test_a_first_call_inside_a_capture_is_refused_and_a_later_one_replays(N=5, D=4, K=2):
    """fastdiff_hip_ext.h: the scratch buffer grows at the first call that needs more, never inside a stream capture.  Assignment and
    record only."""
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: no scratch yet
    lib, h = m._ready(torch.device("cuda"))
    rng = np.random.default_rng(31)
    xa, xb = (torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)).cuda() for _ in range(2))
    cent = torch.from_numpy(rng.standard_normal((K, D)).astype(np.float32)).cuda()
    x = xa.clone()

    def outputs():
        return torch.full((N,), -1, device="cuda", dtype=torch.int32), torch.zeros((dv.RECORD.itemsize,), device="cuda", dtype=torch.uint8)

    def call(rows, assign, rec):
        return lib.fd_bins_pass(h, rows.data_ptr(), N, D, D, None, None, cent.data_ptr(), K, assign.data_ptr(), None, rec.data_ptr(), m._stream(rows.device))

    assign, rec = outputs()
    torch.cuda.synchronize()
    first = torch.cuda.CUDAGraph()
    with torch.cuda.graph(first):
        x.mul_(1.0)                                        # (so that the capture is not empty)
        rc = call(x, assign, rec)
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"stream capture" in msg, (rc, msg)
    torch.cuda.synchronize()
    want = []
    for rows in (xa, xb):                                  # outside: the scratch buffer
        a, r = outputs()
        _capi.check(lib, h, call(rows, a, r), "fd_bins_pass")
        want.append((a, r))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _capi.check(lib, h, call(x, assign, rec), "fd_bins_pass")
    for src, (a, r) in zip((xa, xb), want):
        x.copy_(src)
        assign.fill_(-1)                                   # (the previous assignments are an input: `moved` counts against them)
        rec.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(assign, a) and torch.equal(rec, r) and int(dv._record(rec, K)["counts"].sum()) == N
    assert not torch.equal(want[0][0], want[1][0]) or not torch.equal(want[0][1], want[1][1])


@gpu
def test_rows_that_are_not_finite_are_left_out_and_touch_nothing_else():
    N, D, K = 257, 80, 33
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    at = {5: (0, np.nan), 127: (D - 1, np.inf), 128: (37, -np.inf), 256: (D - 1, np.nan)}          # row -> (feature, value): first, last, interior
    dirty = x.copy()
    for r, (d, v) in at.items():
        dirty[r, d] = v
    keep = np.array([r not in at for r in range(N)])
    got = run_pass(dirty, cent, shift, scale, prev, 96, 1)
    clean = run_pass(x[keep], cent, shift, scale, prev[keep], 96, 1)
    assert (got["assign"][~keep] == -1).all() and (got["assign"][keep] == clean["assign"]).all()
    assert got["rec"]["nonfinite"] == len(at) and got["rec"]["status"] == dv.NONFINITE and clean["rec"]["status"] == dv.OK
    assert got["rec"]["counts"].tobytes() == clean["rec"]["counts"].tobytes() and got["rec"]["counts"].sum() == N - len(at)
    assert got["out"].tobytes() == clean["out"].tobytes()                                           # the sums: bit-identical to the run without those rows
    assert abs(got["rec"]["inertia"] - clean["rec"]["inertia"]) <= 1e-12 * clean["rec"]["inertia"] and got["rec"]["empty"] == clean["rec"]["empty"]
    assert got["rec"]["moved"] == clean["rec"]["moved"] + int((prev[~keep] != -1).sum())
    alone = run_pass(np.full((3, 8), np.nan, np.float32), cent[:2, :8], prev=np.full(3, -1))
    assert alone["rec"]["status"] == dv.EMPTY and alone["rec"]["nonfinite"] == 3 and alone["rec"]["moved"] == 0 and alone["rec"]["empty"] == 2
    assert alone["out"].tobytes() == cent[:2, :8].tobytes() and alone["rec"]["inertia"] == 0.0


@gpu
def test_of_two_identical_centroids_the_lower_index_wins():
    N, D, K = 257, 80, 33
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    twin = cent.copy()
    twin[20], twin[31], twin[32] = cent[3], cent[7], cent[0]          # across the halves of a matrix tile's lanes, and across tiles
    got = run_pass(x, twin, shift, scale, prev)
    base = device(N, D, K, 96, 0)
    for lo, hi in ((3, 20), (7, 31), (0, 32)):
        assert got["rec"]["counts"][hi] == 0 and got["rec"]["counts"][lo] >= base["rec"]["counts"][lo] and (got["assign"] != hi).all()
    assert got["rec"]["counts"][[0, 3, 7]].sum() > 0
    same = run_pass(x, np.repeat(cent[:1], 128, 0), shift, scale, prev, update=False)
    assert (same["assign"] == 0).all()


@gpu
def test_separated_blobs_are_assigned_exactly_as_by_the_oracle():
    for N, D, K in ((257, 36, 33), (C + 1, 80, 50), (300, 128, 128)):
        x, labels = ref.blobs(N + K, N, D, K)
        cent = np.zeros((K, D), np.float32)
        cent[np.arange(K), np.arange(K)] = 19.0
        got = run_pass(x, cent, prev=np.full(N, -1))
        assert (got["assign"] == ref.assign64(x, cent)).all() and (got["assign"] == labels).all() and got["rec"]["moved"] == N


@gpu
def test_the_whole_fit_follows_the_oracle_pass_by_pass():
    x, _ = fit_blobs()
    trail = fit_oracle()
    xd = dev_rows(x)
    cent = torch.from_numpy(trail[0][0]).cuda()
    assign = torch.full((x.shape[0],), -1, dtype=torch.int32, device="cuda")
    for i, (c_ref, r) in enumerate(trail):
        before = cent.cpu().numpy()
        rec, cent = dv.bins_pass(xd, cent, assign=assign, update=True)
        a = assign.cpu().numpy()
        assert (a == r["assign"]).all() and rec["moved"] == r["moved"] and (rec["counts"] == r["counts"]).all(), i
        mean, bound = ref.update_bound(x, a, before, C)
        assert (np.abs(cent.cpu().numpy().astype(np.float64) - mean) <= bound).all(), i
    assert rec["moved"] == 0                                                                          # the same number of passes
    bins = dv.fit(xd, K=5, iters=30, n_init=1, seed=0, standardize=False, check_every=3)
    assert bins.passes == len(trail) and (bins.ref_counts == trail[-1][1]["counts"]).all()
    mean, bound = ref.update_bound(x, trail[-1][1]["assign"], trail[-1][0], C)
    assert (np.abs(bins.centroids.astype(np.float64) - trail[-1][0]) <= 2 * bound).all()
    assert abs(bins.inertia - ref.inertia64(x, bins.centroids, trail[-1][1]["assign"])) <= 1e-12 * bins.inertia


@gpu
def test_inertia_never_rises_by_more_than_the_rows_rounding_bounds():
    N, D, K = 2000, 36, 8
    x, shift, scale, cent, prev, z = inputs(N, D, K)
    xd, sh, sc = dev_rows(x), torch.from_numpy(shift.copy()).cuda(), torch.from_numpy(scale.copy()).cuda()
    cur = torch.from_numpy(z[:K].copy()).cuda()
    assign = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    last = None
    for i in range(12):
        c_in = cur.cpu().numpy()
        rec, cur = dv.bins_pass(xd, cur, sh, sc, assign=assign, update=True)
        slack = float(ref.tau(z, c_in, assign.cpu().numpy())[0].sum())
        print(f"pass {i}: inertia {rec['inertia']:.9g}, moved {rec['moved']}, sum of tau {slack:.3g}")
        assert last is None or rec["inertia"] <= last + slack, i
        last = rec["inertia"]


@gpu
def test_bins_score_the_fitting_set_with_zero_and_a_collapsed_set_as_the_oracle_does():
    x, labels = ref.blobs(21, 1500, 80, 6, sep=6.0)
    xd = dev_rows(x)
    bins = dv.fit(xd, K=6, iters=40, n_init=2, seed=3)
    assert bins.ref_counts.sum() == 1500 and (bins.K, bins.D) == (6, 80)
    own = bins.score(xd)
    assert own["ndb"] == 0 and own["jsd"] == 0.0 and own["n"] == 1500 and (own["counts"] == bins.ref_counts).all()
    z = ref.standardise(x, bins.shift, bins.scale)
    a = ref.assign64(z, bins.centroids)
    assert (np.bincount(a, minlength=6) == bins.ref_counts).all()
    part = x[a >= 3]                                                     # the rows of half the bins removed: a sampler that lost three sounds
    got = bins.score(dev_rows(part, 96, 1), ld=96)
    want = ref.ndb_jsd(bins.ref_counts, np.bincount(a[a >= 3], minlength=6))
    print(f"collapsed: ndb {got['ndb']} / 6, jsd {got['jsd']:.6f}")
    assert got["ndb"] == want["ndb"] >= 3 and abs(got["jsd"] - want["jsd"]) <= 1e-12 and got["n"] == part.shape[0]


@gpu
def test_frames_packs_a_ragged_batch():
    g = torch.Generator().manual_seed(4)
    mels = torch.randn(4, 80, 37, generator=g).cuda()
    lens = (37, 5, 18, 1)
    want = torch.cat([mels[b, :, :n].t() for b, n in enumerate(lens)])
    got = dv.frames(mels, lens)
    assert got.shape == (61, 80) and got.is_contiguous() and torch.equal(got, want)
    assert torch.equal(dv.frames(mels), torch.cat([mels[b].t() for b in range(4)])) and torch.equal(dv.frames(mels[1]), mels[1].t())
    for bad in ((37, 5, 18), (38, 5, 18, 1), (37, -1, 18, 1)):
        with pytest.raises(ValueError):
            dv.frames(mels, bad)


@gpu
def test_fit_bins_of_a_corpus_is_fit_on_its_arena():
    rng = np.random.default_rng(8)
    items = [{"mel": rng.normal(size=(T, 80)).astype(np.float32) + 3 * (i % 2), "wav": np.zeros(T * 256, np.float32), "item_name": f"u{i}"}
             for i, T in enumerate((37, 12, 18))]
    corpus = fastdiff_amd.TrainCorpus(items, max_samples=256 * 4, device="cuda")
    ptr = corpus.mel.data_ptr()
    a = corpus.fit_bins(K=4, iters=20, n_init=2, seed=5)
    b = dv.fit(corpus.mel.clone(), K=4, iters=20, n_init=2, seed=5)
    assert corpus.mel.data_ptr() == ptr and a.ref_counts.sum() == 67
    for name in ("centroids", "shift", "scale", "ref_counts"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert (a.inertia, a.passes) == (b.inertia, b.passes)


@gpu
def test_infer_writes_the_diversity_row(tmp_path):
    from fastdiff_amd import infer
    import synth
    src = tmp_path / "mels"
    src.mkdir()
    mel = synth.synth_mel(5, 2, 40)
    for i in range(2):
        np.save(src / f"u{i}.npy", np.ascontiguousarray(mel[i, :, : 40 - 7 * i].T))
    rows = np.concatenate([mel[0].T, mel[1].T]).astype(np.float32)
    bins = dv.fit(dev_rows(rows), K=4, iters=10, n_init=1)
    bins.save(tmp_path / "bins.npz")
    out = tmp_path / "out"
    with pytest.raises(SystemExit):
        infer.main(["--test_input_dir", str(src), "--out_dir", str(out), "--ndb_bins", str(tmp_path / "bins.npz"), "--out_sample_rate", "16000"])
    infer.main(["--test_input_dir", str(src), "--out_dir", str(out), "--ndb_bins", str(tmp_path / "bins.npz")])
    lines = open(out / "diversity.tsv").read().strip().split("\n")
    assert len(lines) == 2 and lines[0].split("\t") == ["n", "ndb", "ndb_over_k", "jsd"]
    n, ndb, over, jsd = lines[1].split("\t")
    assert int(n) == (1 + 39) + (1 + 32) and 0 <= int(ndb) <= 4 and float(over) == int(ndb) / 4 and 0.0 <= float(jsd) <= np.log(2.0) + 1e-6
    assert sorted(os.listdir(out)) == ["diversity.tsv", "u0.npy_pred.wav", "u1.npy_pred.wav"]
