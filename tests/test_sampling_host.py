"""CPU proofs behind tests/test_sampling_kernels.py: the restatements of tests/sampling_numpy.py are what they claim to be, the GPU
assertions CAN fail (a dropped CDF carry, an unstable rank), and the seeded inputs of tests/sampling_cases.py meet the conditions
the GPU comparisons rest on.  The bounds asserted here are caps set before anything was measured (EXPERIMENTS.md R13 records the
figures); parity.sample_tolerance is used with its existing constants.
"""
import numpy as np
import pytest

import common
import parity
import sampling_cases as SC
import sampling_numpy as SN
from oracle import nsff_oracle as orc

LOOSE_CAP = 0.10            # share of samples whose tolerance exceeds a quarter of the row's mean bin width
DROPPED_CARRY_MIN = 0.5     # share of samples a dropped carry must put outside the tolerance (M > 64)
UNDECIDED_CAP = 0.02        # share of visibility points within the fp32 margin of a decision boundary


def test_sample_pdf64_is_the_oracle_and_the_golden():
    z = np.load(common.GOLDEN_DIR + "/g8_stages.npz")
    bins, w, u40 = z["pdf/bins"], z["pdf/weights"], z["pdf/u_40"]
    u_det = SC.u_shared(64)
    for name, u, want in (("det_64", u_det, z["pdf/det_64"]), ("rand_40", u40, z["pdf/rand_40"])):
        tol = parity.sample_tolerance(bins, w, u)
        got = SN.sample_pdf64(bins, w, u)
        parity.assert_samples_close(f"{name} golden", got, want, tol)
        parity.assert_samples_close(f"{name} oracle", got, orc.sample_pdf(bins, w, u), tol)
        parity.assert_samples_close(f"{name} fp32 scan", SN.sample_pdf32_scan(bins, w, u), got, tol)


def test_cdf32_scan_is_a_cumulative_sum():
    """the restated scan against numpy's cumsum (to fp32 rounding), across the chunk seams; without the carry every chunk restarts"""
    rng = np.random.RandomState(0)
    for M in (1, 63, 64, 65, 129, 257):
        w = (rng.rand(4, M) ** 4).astype(np.float32)
        pdf = (w.astype(np.float64) + 1e-5) / (w.astype(np.float64) + 1e-5).sum(1, keepdims=True)
        want = np.concatenate([np.zeros((4, 1)), np.cumsum(pdf, 1)], 1)
        assert np.abs(SN.cdf32_scan(w) - want).max() < 2e-6
        bad = SN.cdf32_scan(w, carry=False)
        assert np.abs(bad[:, :min(M, 64) + 1] - want[:, :min(M, 64) + 1]).max() < 2e-6
        if M > 64:
            assert np.abs(bad[:, 65] - pdf[:, 64]).max() < 1e-6


@pytest.mark.parametrize("name", list(SC.sampling_cases()))
def test_sampling_case_conditions(name):
    """per case: the fp32 restatement of the kernel's arithmetic is inside parity.sample_tolerance of float64 (the reference
    arithmetic alone passes), with the counting and with the bisecting search; with the carry dropped (M > 64) at least half of the
    samples are outside (counting search; the bisecting one is printed, sampling_numpy.sample_pdf32_scan says why they differ); at
    most 10 % of the samples sit on a tolerance looser than a quarter of the row's mean bin width -- over all rows in the direct
    cases, over the plain rows in the 7-ray cases of the fine table (sampling_cases.py says why no seed holds it over all 7)"""
    worst, used, outside, outside_bisect, loose, total, m_max, loose_plain, total_plain = -np.inf, 0.0, 0, 0, 0, 0, 0, 0, 0
    for bins, w, u, plain in SC.sampling_cases()[name]:
        M = w.shape[1]
        m_max = max(m_max, M)
        tol = parity.sample_tolerance(bins, w, u, SC.EPS)
        want = SN.sample_pdf64(bins, w, u, SC.EPS)
        for search in ("count", "bisect"):
            err = np.abs(SN.sample_pdf32_scan(bins, w, u, SC.EPS, search=search) - want)
            worst, used = max(worst, float((err - tol).max())), max(used, float((err / tol).max()))
        mean_width = (bins[:, -1:] - bins[:, :1]).astype(np.float64) / M
        loose += int((tol > 0.25 * mean_width).sum())
        total += tol.size
        loose_plain += int((tol > 0.25 * mean_width)[plain].sum())
        total_plain += tol[plain].size
        if M > 64:
            bad = SN.sample_pdf32_scan(bins, w, u, SC.EPS, carry=False)
            outside += int((np.abs(bad - want) > tol).sum())
            bad = SN.sample_pdf32_scan(bins, w, u, SC.EPS, carry=False, search="bisect")
            outside_bisect += int((np.abs(bad - want) > tol).sum())
    dropped = f"; outside with the carry dropped {100 * outside / total:.1f} % (bisecting: {100 * outside_bisect / total:.1f} %)"
    print(f"{name}: worst fp32-restatement excess {worst:.3e} ({100 * used:.3f} % of the tolerance used); on loose tolerance "
          f"{100 * loose / total:.2f} % (plain rows: {100 * loose_plain / max(total_plain, 1):.2f} %)" + (dropped if m_max > 64 else ""))
    assert worst <= 0, f"{name}: the fp32 restatement leaves the tolerance by {worst:.3e}"
    if name.startswith("pdf"):
        assert loose <= LOOSE_CAP * total, f"{name}: {loose} of {total} samples on a loose tolerance"
    else:                       # 4 of the 7 rays are special rows, loose by construction (sampling_cases.py): the cap is held on the others
        assert (total_plain > 0 or m_max == 1) and loose_plain <= LOOSE_CAP * total_plain, f"{name}: {loose_plain} of {total_plain}"
        assert m_max > 1 or loose == 0                        # (one bin: every row is its own spike, and none is loose)
    if m_max > 64:
        assert outside >= DROPPED_CARRY_MIN * total, f"{name}: a dropped carry moves only {outside} of {total} samples outside"
        # the GPU test allows no sample outside: a bisecting kernel without the carry fails the direct test at every M > 64 too
        assert outside_bisect > 0 or not name.startswith("pdf")


def test_special_rows_are_present():
    for M in SC.PDF_M:
        names = [n for n, _ in SC.special_rows(M)]
        assert names == ["zero", "first", "last"] + (["seam"] if M > 64 else [])
        for n_rays in (5, 37):
            w = SC.pdf_case(M, n_rays, 64).weights
            for r, (_, spike) in enumerate(SC.special_rows(M)):
                want = np.zeros(M, np.float32)
                if spike is not None:
                    want[spike] = 1
                assert np.array_equal(w[r], want)
        singles = {tuple(SC.pdf_case(M, 1, k).weights[0]) for k in SC.PDF_IMP}
        assert len(singles) == len({spike for _, spike in SC.special_rows(M)})       # the single-ray launches rotate through all of them
    for S, n_imp, sets in SC.FINE_TABLE:
        c = SC.fine_case(S, n_imp, sets)
        inner = np.concatenate([w[:, 1:-1] for w in c.w], 0)
        rows = {tuple(r) for r in inner}
        for _, spike in SC.special_rows(c.M):
            want = np.zeros(c.M, np.float32)
            if spike is not None:
                want[spike] = 1
            assert tuple(want) in rows, (S, spike)
        assert c.Sf == S + sets * n_imp and c.zs_coarse.shape == (SC.FINE_RAYS, S)
        assert (np.diff(c.zs_coarse, axis=1) >= 0).all()


def test_fine_table_reaches_the_named_routes():
    shapes = {(S, n_imp, sets): (S - 2, S + sets * n_imp) for S, n_imp, sets in SC.FINE_TABLE}
    assert shapes[(3, 1, 1)] == (1, 4)
    assert shapes[(65, 17, 1)] == (63, 82) and 82 % 4 == 2 and 65 % 4 == 1
    assert shapes[(67, 5, 2)] == (65, 77) and 77 % 4 == 1
    assert shapes[(66, 33, 2)] == (64, 132)
    assert shapes[(128, 128, 2)] == (126, 384)
    assert shapes[(130, 64, 1)][0] == 128
    assert shapes[(257, 3, 2)] == (255, 263)


@pytest.mark.parametrize("shape", SC.TIE_TABLE, ids=str)
def test_rank_sort_mutation_leaves_a_slot_unwritten(shape):
    """on the tie rows the stable rank equals np.sort and the unstable one leaves NaN; without ties both equal np.sort"""
    c = SC.fine_case(*shape, ties=True)
    samples = [SN.sample_pdf32_scan(c.mids, c.w[k][:, 1:-1], c.u["shared"][k], SC.EPS) for k in range(c.sets)]
    merged = np.concatenate([c.zs_coarse] + samples, 1)
    assert merged.shape[1] == c.Sf
    # the ties are there: all coarse depths equal / n_imp exact pairs / a coarse depth equal to the u = 0 sample of both sets
    assert np.unique(merged[SC.TIE_SAME, :c.S]).size == 1
    assert np.array_equal(samples[0][SC.TIE_ZERO], samples[1][SC.TIE_ZERO])
    assert np.unique(samples[0][SC.TIE_ZERO]).size == c.n_imp
    edge = merged[SC.TIE_EDGE]
    assert edge[SC.TIE_EDGE_AT] == c.mids[0, 0] == samples[0][SC.TIE_EDGE, 0] == samples[1][SC.TIE_EDGE, 0]
    stable = SN.rank_sort(merged)
    assert np.array_equal(stable, np.sort(merged, 1))
    unstable = SN.rank_sort(merged, stable=False)
    for ray in (SC.TIE_SAME, SC.TIE_ZERO, SC.TIE_EDGE):
        assert np.isnan(unstable[ray]).any(), ray
    plain = [r for r in range(SC.FINE_RAYS) if np.unique(merged[r]).size == c.Sf]
    assert np.array_equal(unstable[plain], np.sort(merged[plain], 1))


@pytest.mark.parametrize("S,n_imp,sets", SC.FINE_TABLE)
def test_rank_sort_equals_np_sort_on_every_row(S, n_imp, sets):
    c = SC.fine_case(S, n_imp, sets)
    for form in ("shared", "per_ray"):
        samples = [SN.sample_pdf32_scan(c.mids, c.w[k][:, 1:-1], c.u[form][k], SC.EPS) for k in range(sets)]
        merged = np.concatenate([c.zs_coarse] + samples, 1)
        assert np.array_equal(SN.rank_sort(merged), np.sort(merged, 1))


def test_coarse32_is_the_oracle_stratified_sampling():
    """coarse32 against the reference's formula (rendering.py:314-324) evaluated in float64"""
    for S in SC.COARSE_S:
        c = SC.coarse_case(S, 5)
        z = c.z_lin.astype(np.float64)
        mid = 0.5 * (z[:-1] + z[1:])
        lower, upper = np.concatenate([z[:1], mid]), np.concatenate([mid, z[-1:]])
        for perturb in SC.COARSE_PERTURB:
            zs, xyz = SN.coarse32(c.rays, c.z_lin, perturb, c.rnd)
            want = lower + (upper - lower) * (perturb * c.rnd.astype(np.float64)) if perturb > 0 else np.broadcast_to(z, (5, S))
            assert zs.dtype == np.float32 and np.abs(zs - want).max() < 3e-7
            pts = c.rays[:, None, :3].astype(np.float64) + c.rays[:, None, 3:].astype(np.float64) * want[..., None]
            assert xyz.dtype == np.float32 and np.abs(xyz - pts).max() < 1e-6


@pytest.mark.parametrize("n_cams", SC.VIS_CAMS)
def test_visibility_inputs_meet_their_conditions(n_cams):
    """every count 0 .. n_cams occurs; at most 2 % of the points are undecided; on the decided ones the fp32 oracle (ndc_to_world +
    world_visibility summed over the cameras) equals frustum_count64 exactly; a frame outside the table is seen by nobody"""
    for frame in SC.vis_frames(SC.VisDataset(n_cams).N_frames):
        c = SC.vis_case(n_cams, frame)
        ds = c.dataset
        assert set(np.unique(c.counts)) == set(range(n_cams + 1)), np.unique(c.counts)
        share = c.undecided.mean()
        print(f"n_cams={n_cams} frame={frame}: counts {np.bincount(c.counts.astype(int))}, undecided {100 * share:.2f} %")
        assert share <= UNDECIDED_CAP
        world = orc.ndc_to_world(c.points, c.K)
        with np.errstate(all="ignore"):
            o32 = sum(orc.world_visibility(world, c.K, ds.img_wh[1], ds.img_wh[0], ds.poses[i * ds.N_frames + frame])
                      for i in range(n_cams))
        keep = ~c.undecided
        assert np.array_equal(o32[keep], c.counts[keep])
        assert (c.points[:, 2] > 1).any() and (c.points[:, 2] == 1).any()
        for P in SC.VIS_P:
            assert P <= c.points.shape[0]
    for frame in (-1, SC.VisDataset(n_cams).N_frames):
        c = SC.vis_case(n_cams, frame)
        assert not c.counts.any() and np.isinf(c.margins).all()


def test_warp32_takes_the_strict_comparison():
    for P in SC.WARP_P:
        c = SC.warp_case(P)
        fw, bw = SN.warp32(c.raw, c.xyz, c.zs, SC.WARP_Z_FAR)
        at, above = c.zs == np.float32(SC.WARP_Z_FAR), c.zs == np.nextafter(np.float32(SC.WARP_Z_FAR), np.float32(2))
        assert at[0::3].all() and above[1::3].all() and not (at & above).any()
        assert np.array_equal(fw[at], c.xyz[at] + c.raw[at, 8:11]) and np.array_equal(bw[at], c.xyz[at] + c.raw[at, 11:14])
        assert np.array_equal(fw[above], c.xyz[above]) and np.array_equal(bw[above], c.xyz[above])
        assert (3 * P - 1) // 256 == {1: 0, 85: 0, 86: 1, 1000: 11}[P]
