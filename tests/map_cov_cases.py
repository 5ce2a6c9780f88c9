"""Inputs of the map-covariance tests (tests/test_gpu_map_cov.py): small noisy blocks cut from map_robust_cases' and
map_rig_cases' blocks, so that the number of tags besides the world tag sits on either side of the covariance kernels' edges:
6 n = 6, 42, 48, 54, 96 and 102 against GN_NB = 48 (the factor's block), the 16-wide MFMA blocks and the 32-wide tiles of
k_map_cov_gram."""
import functools

import numpy as np

import map_rig_cases as MRC
import map_robust_cases as MBC

TAG_COUNTS = (1, 7, 8, 9, 16, 17)
N_FRAMES = 5


def keep_ids(obs, ids):
    out = obs.copy()
    m = ~np.isin(out["id"], ids)
    out["id"][m], out["flags"][m] = -1, 0
    return out


@functools.lru_cache(maxsize=None)
def tag_count_block(n):
    """(N_FRAMES, 24) records with corner noise that see the n + 1 lowest ids of the bench scene: n tags besides the world tag"""
    obs, _, _ = MBC.noisy_block(N_FRAMES, 24)
    ids = sorted({int(i) for i in obs["id"].ravel() if i >= 0})
    assert len(ids) > n
    return keep_ids(obs, ids[:n + 1])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (obs, rig or None, dist, huber_px, tag_sizes): one camera's (n_frames, max_tags) or a rig's camera-major block"""
    out = {"tags_%d" % n: (tag_count_block(n), None, None, 0.0, None) for n in TAG_COUNTS}
    out["behind"] = (MBC.behind_case(), None, None, MBC.HUBER, None)                # a tag the behind test leaves without a view
    out["huber_dist5"] = (MBC.repair_cases()["dist5_swap"][0][3:9], None, MBC.MC.DIST5, MBC.HUBER, None)
    out["sized"] = (tag_count_block(8), None, None, 0.0, {1: MBC.LC.TAG_INNER})     # a table entry equal to the call's size
    out["rig_pair"] = (MRC.pair_block(6, 12, MRC.NOISE), MRC.PAIR, None, 0.0, None)  # (frame, tag) pairs with two views
    out["nothing"] = (MBC.empty_frames(3, 4), None, None, 0.0, None)                # status 1: no slot, every cov_slot -1
    return out
