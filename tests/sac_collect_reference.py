"""tb_sac_collect's uniform mode restated in numpy over policy_reference.philox4x32: action k of (seed, env, episode, step) is
(float32)(w >> 8) * 2^-23 - 1 with w = word k % 4 of the Philox block k / 4 that policy_noise keys its normals by. Every operation
is exact in float32: w >> 8 < 2^24 is a float32 integer, the scaling is by a power of two, and the difference is a multiple of
2^-23 of magnitude <= 1."""
import numpy as np

import policy_reference as pr


def uniform_actions(seed, env_id, episode, step_count, n_act):
    """float32 [..., n_act]; env_id, episode, step_count broadcast against each other"""
    env_id, episode, step_count = np.broadcast_arrays(np.asarray(env_id, np.uint64), np.asarray(episode, np.uint64),
                                                      np.asarray(step_count, np.int64).astype(np.uint64) & np.uint64(pr.M32))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (np.uint64(seed & pr.M32), np.uint64((seed >> 32) ^ pr.NOISE_KEY_TAG))
    m = np.uint64(pr.M32)
    out = []
    for blk in range((n_act + 3) // 4):
        ctr = (env_id & m, env_id >> np.uint64(32), episode & m, (step_count * np.uint64(4) + np.uint64(blk)) & m)
        for w in pr.philox4x32(ctr, key):
            top = (np.asarray(w, np.uint64) >> np.uint64(8)).astype(np.float32)        # < 2^24: exact
            out.append(top * np.float32(2.0 ** -23) - np.float32(1.0))                 # float32 all the way
    return np.stack(out[:n_act], -1)
