"""The NumPy statement of the pose covariance (tests/pose_cov_ref.py, through localize_ref.pose_cov) against what it
claims: the convention map against finite differences of the pose composition itself, and the covariance against the
scatter of solved poses around the truth under corner noise of a known sigma."""
import numpy as np

import localize_cases as LC
import localize_ref as LR
import pose_cov_ref as PC
from aprilslam_amd import synth
from aprilslam_amd.localize import TagMap

K = synth.camera_matrix(LC.W, LC.H, 45.0)
CAM = LR.camera(K, None)
ONE = LR.OneCamera(CAM)
N_TRIALS = 500
BOUND = 5 * np.sqrt(12.0 / N_TRIALS)    # chi-square(6): variance 12; five standard errors of the mean of N_TRIALS


def multi_tag_scene():
    """frame 3 of the bench trajectory over the 20-tag bench scene: (R, t) camera<-world, world corners, true pixels"""
    tags = LC.bench_scene()
    rec = TagMap.from_scene(tags).as_records()
    pos, rot = LC.trajectory(16)[3]
    obs = LC.exact_frame(tags, pos, rot, K)
    slots = [s for s in range(len(obs)) if obs["id"][s] >= 0]
    assert len(slots) >= 6
    Xw, _, _ = LR.frame_points(ONE, obs, rec, LC.TAG_INNER, slots)
    Tcw = np.linalg.inv(LC.world_from_camera(pos, rot))
    R, t = Tcw[:3, :3], Tcw[:3, 3]
    return R, t, Xw, LR.project(CAM, Xw @ R.T + t)


def single_tag_scene():
    """one tag of side 10 seen from 40 units at 45 degrees about an axis in its plane (about 190 px across): large and
    oblique, so that the second planar minimum is far and the linearisation holds at 0.2 px (a small frontal tag at
    0.3 px has heavy tails).  The map is that tag at the identity: camera<-world is camera<-tag."""
    R = LR.rodrigues(np.array([0.6, -0.5, 0.2]) / np.sqrt(0.65) * np.radians(45.0)) @ np.diag([1.0, -1.0, -1.0])
    t = np.array([3.0, -2.0, 40.0])
    Xw = np.c_[LR.object_corners(LC.TAG_INNER), np.zeros(4)]
    return R, t, Xw, LR.project(CAM, Xw @ R.T + t)


def test_convention_map_against_finite_differences():
    rng = np.random.default_rng(7)
    h = 1e-6
    for wfc in (True, False):
        for _ in range(5):
            R = LR.rodrigues(rng.normal(size=3))
            t = rng.normal(size=3) * np.array([20.0, 20.0, 100.0])
            A = PC.convention_map(R, t, wfc)
            Ro, p = PC.output_pose(R, t, wfc)
            fd = np.zeros((6, 6))
            for k in range(6):
                e = []
                for sgn in (1.0, -1.0):
                    delta = np.zeros(6)
                    delta[k] = sgn * h
                    dR = LR.rodrigues(delta[:3])
                    Rn, pn = PC.output_pose(dR @ R, dR @ t + delta[3:], wfc)    # the solvers' own update, then the pose handed out
                    e.append(PC.pose_error(Ro, p, Rn, pn))
                fd[:, k] = (e[0] - e[1]) / (2 * h)
            assert np.abs(fd - A).max() <= 1e-6 * np.abs(A).max(), (wfc, np.abs(fd - A).max(), np.abs(A).max())


def mahalanobis_trials(scene, sigma, wfc, seed, sigma_arg):
    """N_TRIALS noisy solves from the true pose: squared Mahalanobis distance of each solution's (r, d) error under the
    covariance predicted at that solution, and the sigma each prediction used"""
    R0, t0, Xw, uv0 = scene
    Rt, pt = PC.output_pose(R0, t0, wfc)
    rng = np.random.default_rng(seed)
    m2, sig = [], []
    for _ in range(N_TRIALS):
        uv = uv0 + rng.normal(scale=sigma, size=uv0.shape)
        R, t, _ = LR.lm(LR.corner_lin(CAM, Xw, uv), R0.copy(), t0.copy())
        C, s, dof, status = LR.pose_cov(ONE, R, t, Xw, uv, None, sigma_arg, wfc)
        assert status == 0 and dof == 2 * len(Xw) - 6
        Re, pe = PC.output_pose(R, t, wfc)
        e = PC.pose_error(Re, pe, Rt, pt)
        m2.append(float(e @ np.linalg.solve(C, e)))
        sig.append(s)
    return np.array(m2), np.array(sig)


def test_covariance_is_consistent_with_the_scatter_multi_tag():
    """world<-camera over the mapped tags of a bench frame, 0.3 px corner noise, sigma given"""
    m2, sig = mahalanobis_trials(multi_tag_scene(), 0.3, True, 101, 0.3)
    print("multi-tag: mean squared Mahalanobis distance %.3f (6 +- %.2f)" % (m2.mean(), BOUND))
    assert np.all(sig == 0.3)
    assert abs(m2.mean() - 6.0) <= BOUND, m2.mean()


def test_covariance_is_consistent_with_the_scatter_single_tag():
    """camera<-tag of one large oblique tag (single_tag_scene), 0.2 px corner noise, sigma given"""
    m2, _ = mahalanobis_trials(single_tag_scene(), 0.2, False, 202, 0.2)
    print("single tag: mean squared Mahalanobis distance %.3f (6 +- %.2f)" % (m2.mean(), BOUND))
    assert abs(m2.mean() - 6.0) <= BOUND, m2.mean()


def test_estimated_sigma_multi_tag():
    """sigma_px = 0: the mean of cost / dof's root over the trials against the true sigma, five standard errors"""
    scene = multi_tag_scene()
    dof = 2 * len(scene[2]) - 6
    _, sig = mahalanobis_trials(scene, 0.3, True, 303, 0.0)
    se = 0.3 / np.sqrt(2.0 * dof * N_TRIALS)
    print("estimated sigma: mean %.5f (0.3 +- %.5f), dof %d" % (sig.mean(), 5 * se, dof))
    assert abs(sig.mean() - 0.3) <= 5 * se, (sig.mean(), se)


def test_status_1_and_2_give_zeros():
    C, s, dof, status = PC.no_pose(0.5)
    assert status == 1 and dof == 0 and s == 0.5 and not C.any()
    # every corner on one ray: all rows of J alike per corner, J^T J has rank 2
    R, t = np.eye(3), np.array([0.0, 0.0, 50.0])
    Xw = np.tile(np.array([[1.0, 2.0, 0.0]]), (8, 1))
    uv = LR.project(CAM, Xw @ R.T + t) + 0.1
    for wfc in (True, False):
        C, s, dof, status = LR.pose_cov(ONE, R, t, Xw, uv, None, 0.5, wfc)
        assert status == 2 and dof == 10 and not C.any()
    R, t, Xw, uv = multi_tag_scene()
    C, s, dof, status = LR.pose_cov(ONE, R, t, Xw, uv, None, 0.5, True)
    assert status == 0 and (np.diag(C) > 0).all()
    assert np.abs(C - C.T).max() <= 1e-12 * np.abs(C).max()
