"""What the map-covariance entry points say when they refuse (check_map_call, csrc/solve_host.inc), in
test_gpu_solver_refusals.py's way and with its tools: the valid call returns 0, every single-fault call returns -1 with the
literal asl_last_error() text and writes nothing, a two-fault call gives the message of the check that comes first, and the
host and device forms say the same.  The order: the sized form's refusals where they stand, the NULL covariance outputs
with the other NULL arguments, cap_tags after tag_sizes and before a rig's table.  (More tags than cap_tags is known only
after the gather: tests/test_gpu_map_cov.py.)"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_solver_refusals import (DIST, MAX_TAGS, MT, N, N_DIST, N_IDS, NI, NO_DIST, NULL_ARG, NULL_D, TAG_SIZE, K, Form, block, both, dptr,  # noqa: F401
                                      faults, run)

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
KEEP = []


def fptr(*v):
    KEEP.append(np.array(v, dtype=np.float32))
    return KEEP[-1].ctypes.data_as(FP)


@pytest.mark.parametrize("rig", [False, True])
def test_map_cov(block, rig):
    said = {}
    for device, src in both(block):
        tmap, std, poses, res = block.out(NI * 104, device), block.out(NI * 48, device), block.out(N * 160, device), block.out(64, device)
        weight, slot, cov = block.out(N * MT * 8, device), block.out(NI * 4, device), block.out(36 * 8, device)
        base = dict(d=block.h, obs=block.ptr(src["obs"]), n_frames=N, max_tags=MT, n_ids=NI, tag_size=0.1, tag_sizes=None, world_id=-1, huber_px=0.0,
                    max_iters=2, map=block.ptr(tmap), tag_std=block.ptr(std), poses=block.ptr(poses), result=block.ptr(res),
                    slot_weight=block.ptr(weight), cov_slot=block.ptr(slot), map_cov=block.ptr(cov), cap_tags=1)
        tail = "tag_size tag_sizes world_id huber_px max_iters map tag_std poses result slot_weight cov_slot map_cov cap_tags"
        if rig:
            base.update(n_cams=1, rig=block.ptr(src["rig"]))
            names = "d obs n_cams n_frames max_tags n_ids rig " + tail
        else:
            base.update(K=dptr(K), dist=None, n_dist=0)
            names = "d obs n_frames max_tags n_ids K dist n_dist " + tail
        if device:
            base["stream"] = None
            names += " stream"
        form = Form("asl_mapcov%s_%s" % ("_rig" if rig else "", "frames_device" if device else "batch"), names, base,
                    [tmap, std, poses, res, weight, slot, cov])
        world, iters = "world_id must be -1 or in [0, n_ids) (got %d)", "max_iters must be in [1, 1000] (got %d)"
        huber, sizes, cap = "huber_px must be >= 0 and finite (got -1)", "tag_sizes[0] must be 0 or positive and finite (got -1)", "cap_tags must be >= 1 (got %d)"
        single = [(NULL_D, dict(d=None)), (NULL_ARG, dict(obs=None)), (NULL_ARG, dict(map=None)), (NULL_ARG, dict(poses=None)),
                  (NULL_ARG, dict(result=None)), (NULL_ARG, dict(cov_slot=None)), (NULL_ARG, dict(map_cov=None)),
                  ("n_frames must be >= 1 (got 0)", dict(n_frames=0)), (MAX_TAGS % 257, dict(max_tags=257)), (N_IDS, dict(n_ids=0)),
                  (TAG_SIZE, dict(tag_size=0.0)), (world % 1, dict(world_id=1)), (iters % 0, dict(max_iters=0)), (huber, dict(huber_px=-1.0)),
                  (sizes, dict(tag_sizes=fptr(-1.0))), (cap % 0, dict(cap_tags=0)), (cap % -3, dict(cap_tags=-3))]
        pairs = [(NULL_ARG, dict(map_cov=None, n_frames=0)), ("n_frames must be >= 1 (got 0)", dict(n_frames=0, cap_tags=0)),
                 (sizes, dict(tag_sizes=fptr(-1.0), cap_tags=0)), (huber, dict(huber_px=-1.0, cap_tags=0)), (NULL_D, dict(d=None, cov_slot=None))]
        if rig:
            single += [(NULL_ARG, dict(rig=None)), ("n_cams must be in [1, 16] (got 17)", dict(n_cams=17))]
            bad = block.host["rig"].copy()
            bad["n_dist"] = 3
            bad_p = bad.ctypes.data
            if device:
                import torch
                KEEP.append(torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).to("cuda:0"))
                bad_p = KEEP[-1].data_ptr()
            else:
                KEEP.append(bad)
            pairs += [(cap % 0, dict(cap_tags=0, rig=bad_p))]                                 # cap_tags comes before the table
            single += [("camera 0: n_dist must be 0, 4 or 5 (got 3)", dict(rig=bad_p))]
        else:
            single += [(NULL_ARG, dict(K=None)), (N_DIST, dict(n_dist=3, dist=dptr(DIST))), (NO_DIST, dict(n_dist=4))]
        run(form, single, pairs)
        said[device] = faults(single + pairs)
    assert said[True] == said[False]


@pytest.mark.parametrize("rig", [False, True])
def test_localize_mapcov(block, rig):
    """asl_localize_mapcov_* / asl_localize_rig_mapcov_*: the _cov form's refusals where they stand, then the covariance's
    pointers and ld, then (host forms) the look into cov_slot and the blocks, a rig's table last"""
    said = {}
    for device, src in both(block):
        out, cov = block.out(N * 160, device), block.out(N * 304, device)
        slot_h, mat_h = np.full(NI, -1, dtype=np.int32), np.zeros((6, 6))
        KEEP.extend([slot_h, mat_h])
        if device:
            import torch
            KEEP.extend([torch.from_numpy(slot_h).to("cuda:0"), torch.from_numpy(mat_h).to("cuda:0")])
            slot_p, mat_p = KEEP[-2].data_ptr(), KEEP[-1].data_ptr()
        else:
            slot_p, mat_p = slot_h.ctypes.data, mat_h.ctypes.data
        base = dict(d=block.h, obs=block.ptr(src["obs"]), n_frames=N, max_tags=MT, map=block.ptr(src["map"]), n_ids=NI, tag_size=0.1, gate=0.0, sigma_px=0.0,
                    out=block.ptr(out), cov=block.ptr(cov), map_cov=mat_p, ld=6, cov_slot=slot_p)
        tail = "tag_size gate sigma_px out cov map_cov ld cov_slot"
        if rig:
            base.update(n_cams=1, rig=block.ptr(src["rig"]))
            names = "d obs n_cams n_frames max_tags map n_ids rig " + tail
        else:
            base.update(K=dptr(K), dist=None, n_dist=0)
            names = "d obs n_frames max_tags map n_ids K dist n_dist " + tail
        if device:
            base["stream"] = None
            names += " stream"
        form = Form("asl_localize%s_mapcov_%s" % ("_rig" if rig else "", "frames_device" if device else "batch"), names, base, [out, cov])
        gate, sigma, ld = "max_tag_rms_px must be >= 0 (got -1)", "sigma_px must be >= 0 and finite (got -1)", "ld must be a positive multiple of 6 (got %d)"
        single = [(NULL_ARG, dict(cov=None)), (NULL_D, dict(d=None)), (NULL_ARG, dict(out=None)), (NULL_ARG, dict(map=None)),
                  ("n_frames < 0", dict(n_frames=-1)), (MAX_TAGS % 257, dict(max_tags=257)), (N_IDS, dict(n_ids=0)), (TAG_SIZE, dict(tag_size=0.0)),
                  (gate, dict(gate=-1.0)), (sigma, dict(sigma_px=-1.0)), (NULL_ARG, dict(map_cov=None)), (NULL_ARG, dict(cov_slot=None)),
                  (ld % 0, dict(ld=0)), (ld % 7, dict(ld=7)), (ld % -6, dict(ld=-6))]
        pairs = [(NULL_ARG, dict(cov=None, d=None)), (sigma, dict(sigma_px=-1.0, map_cov=None)), (NULL_ARG, dict(cov_slot=None, ld=0)),
                 (gate, dict(gate=-1.0, ld=7))]
        if rig:
            single += [(NULL_ARG, dict(rig=None)), ("n_cams must be in [1, 16] (got 17)", dict(n_cams=17))]
        else:
            single += [(NULL_ARG, dict(K=None)), (N_DIST, dict(n_dist=3, dist=dptr(DIST))), (NO_DIST, dict(n_dist=4))]
        run(form, single, pairs)
        said[device] = faults(single + pairs)
        if not device:    # what only the host form can see before the launch
            bad_slot, nan_mat = np.array([1], dtype=np.int32), np.full((6, 6), np.nan)
            KEEP.extend([bad_slot, nan_mat])
            form.fill()
            form.refuses("cov_slot[0] must be in [-1, 1) (got 1)", cov_slot=bad_slot.ctypes.data)
            form.refuses("cov_slot[0] must be in [-1, 1) (got -2)", cov_slot=_keep(np.array([-2], dtype=np.int32)))
            form.refuses("map_cov is not finite at (0, 0)", cov_slot=_keep(np.array([0], dtype=np.int32)), map_cov=nan_mat.ctypes.data)
            assert form.untouched()
    assert said[True] == said[False]


def _keep(a):
    KEEP.append(a)
    return a.ctypes.data


def test_sizes():
    """the argument lists are the sized forms' with the three covariance arguments after slot_weight"""
    L = _lib_load()
    for rig in ("", "_rig"):
        sized_dev, sized_host = getattr(L, "asl_map%s_sized_frames_device" % rig).argtypes, getattr(L, "asl_map%s_sized_batch" % rig).argtypes
        cov_dev, cov_host = getattr(L, "asl_mapcov%s_frames_device" % rig).argtypes, getattr(L, "asl_mapcov%s_batch" % rig).argtypes
        assert list(cov_host) == list(sized_host) + [C.c_void_p, C.c_void_p, C.c_int]
        assert list(cov_dev) == list(sized_dev[:-1]) + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        plain_dev, plain_host = getattr(L, "asl_localize%s_cov_frames_device" % rig).argtypes, getattr(L, "asl_localize%s_cov_batch" % rig).argtypes
        mc_dev, mc_host = getattr(L, "asl_localize%s_mapcov_frames_device" % rig).argtypes, getattr(L, "asl_localize%s_mapcov_batch" % rig).argtypes
        assert list(mc_host) == list(plain_host) + [C.c_void_p, C.c_int, C.c_void_p]
        assert list(mc_dev) == list(plain_dev[:-1]) + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    from aprilslam_amd import _lib
    assert _lib.POSE_COV_DTYPE.itemsize == 304      # the record is unchanged: status 3 is a new value of its status field


def _lib_load():
    from aprilslam_amd import _lib
    return _lib.load()
