"""fp64 restatement of HumanoidAREnv.get_ar_obs_v1 (kin_poly/envs/humanoid_ar_v1.py:133-214) under the statear switches use_vel / use_head /
use_action (use_obj on; use_of, use_context off), written from the reference's block list (:183-201):

    curr_qpos_local[2:]                          74   always
    curr_qvel = data.qvel[:75]                   75   use_vel
    diff_hpos, diff_hrot                          7   use_head
    pred_obj_relative_head                        7   always
    t_havel, t_hlvel, t_obj_relative_head        13   use_head
    curr_action                                   4   use_action

Test infrastructure (a sibling of oracle/np_oracle.py, whose quaternion helpers it uses); held to tests/golden/ar_obs_variants.npz, which
tools/make_golden_obs_variants.py writes by running the reference itself."""
import numpy as np

from oracle import np_oracle as O

VARIANTS = [(v, h, a) for h in (True, False) for v in (False, True) for a in (True, False)]      # (use_vel, use_head, use_action), the issue's table order
NEW_VARIANTS = [s for s in VARIANTS if s[0] or not s[1]]                                             # without kin_poly.yml's 105 / 101


def key(vel, head, action):
    return f"v{int(vel)}h{int(head)}a{int(action)}"


def width(vel, head, action):
    return 74 + 75 * bool(vel) + 7 * bool(head) + 7 + 13 * bool(head) + 4 * bool(action)


def offsets(vel, head, action):
    """first column of every block: dict(pose, vel, diff, obj, tgt, act, end); an absent block has the offset of the block after it"""
    o = dict(pose=0, vel=74)
    o["diff"] = o["vel"] + 75 * bool(vel)
    o["obj"] = o["diff"] + 7 * bool(head)
    o["tgt"] = o["obj"] + 7
    o["act"] = o["tgt"] + 13 * bool(head)
    o["end"] = o["act"] + 4 * bool(action)
    return o


def obs_ar_variant(qpos, qvel, xpos, xquat, head_pose_t, head_vels_t, obj_rel_t, action_one_hot, obj_qpos7, use_vel=False, use_head=True, use_action=True,
                   head_idx=13):
    curr = np.array(qpos, float)
    curr[3:7] = O.de_heading(curr[3:7])
    pred_hrot, pred_hpos = np.asarray(xquat, float)[head_idx], np.asarray(xpos, float)[head_idx]
    obs = [curr[2:]]
    if use_vel:
        obs.append(np.array(qvel, float)[:75])
    if use_head:
        obs.append(O.transform_vec(head_pose_t[:3] - pred_hpos, pred_hrot, "heading"))
        obs.append(O.quaternion_multiply(O.quaternion_inverse(head_pose_t[3:]), pred_hrot))
    obj = np.array([0, 0, 0, 1, 0, 0, 0.0]) if np.sum(action_one_hot) == 0 else np.asarray(obj_qpos7, float)          # get_obj_qpos (:465-466)
    obs.append(O.transform_vec(obj[:3] - pred_hpos, pred_hrot, "heading"))
    obs.append(O.quaternion_multiply(O.quaternion_inverse(O.get_heading_q(pred_hrot)), obj[3:7]))
    if use_head:
        obs += [head_vels_t[3:], head_vels_t[:3], obj_rel_t]
    if use_action:
        obs.append(action_one_hot)
    return np.concatenate(obs)
