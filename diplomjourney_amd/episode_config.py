"""What the host and the device episodes share: the episode configs
(mpc_episode_config_t) and the device episode's chain errors."""
import math

from . import math_model_tree as mmt
from .abi import MpcEpisodeConfig

CHAIN_ERRORS = {
    1: "a chained launch's tile blocks timed out waiting for block 0's published constants "
       "(the step was scored on speculated constants)",
    2: "the state was reset with another wheelbase form (power of two or not) than the "
       "launch's cfg",
    3: "an exchange launch's block 0 timed out collecting its tile records (this rank's "
       "candidate dropped out of the global arg-min)",
    4: "an overlapped exchange launch's block 0 timed out waiting for the all_gather's mark "
       "(the collective could not run beside the launch: the step was not completed)",
    5: "a P2P exchange launch's block 0 timed out waiting for the ranks' candidates in its "
       "mailbox (a peer did not run the same step: the step was not completed)",
    6: "a one-GPU chained step's early publication of the next step's constants disagreed "
       "with its update (a self-check: never expected)",
}


class ChainError(RuntimeError):
    """A device-resident episode's bounded wait failed (EpisodeState::chain_error)."""

    def __init__(self, code):
        self.code = int(code)
        super().__init__(f"chain_error {self.code}: {CHAIN_ERRORS.get(self.code, 'unknown')}")


def reference_episode_config(start=(0.0, 0.0, 0.0, 0.0, 0.0), target=(2, 3), seed=20261015,
                             max_steps=0, incumbent0=0.0, enumerate=False):
    """mpc_episode_config_t with the reference's constants and expressions
    (config.py; grid ratios as math_model_tree.py:241-253 computes them; the
    operator schedule of :564-569; slow_down bands of :219-226).  max_steps 0:
    no step limit (the reference's loop runs until on target or stuck);
    incumbent0 0: the first incumbent from the episode's target (the
    reference's, 10000050990.195135, is config.py's target's, :676);
    enumerate: sampled steps hold exactly the step's |V|*|B| constant
    sequences (the reference's candidate set), the rest padding."""
    c = mmt._cfg
    return MpcEpisodeConfig(
        start_x=start[0], start_y=start[1], start_phi=start[2], start_v=start[3],
        start_beta=start[4], target_x=target[0], target_y=target[1],
        L=c.L, delta_t=c.delta_t, eps=c.eps, v_max=c.v_max, v_min=c.v_min, delta_v=c.delta_v,
        ratio_v=(c.v_acc_max * c.delta_t) / c.delta_v, delta_beta=c.delta_beta,
        ratio_beta=(math.degrees(c.beta_acc_max) * c.delta_t) / math.degrees(c.delta_beta),
        beta_bound=c.beta_max + math.radians(c.eps_beta), radius_u_turn=mmt.radius_u_turn,
        turn_distance=2.0, event_target_x=2.0, event_target_y=3.0,
        p_turn_right=60, p_turn_left=90, p_new_target=110, slow_new_target=10, slow_turn=20,
        max_steps=max_steps, incumbent0=incumbent0, enumerate=int(bool(enumerate)), seed=seed)


def tree_episode_config(start, max_calls=None):
    """mpc_episode_config_t of one run_math_model.py episode (:231-280) whose
    MPC step is math_model_tree.py's tree expansion (SURVEY Fact 2): start =
    (x_0, y_0, phi_0, x_t, y_t) as draw_starts() draws them, v = beta = 0
    (:233-234); the reference's grid constants and enumeration; the first
    incumbent from the start with the episode's target (:252); no operator
    events; the script's stuck rule (the second non-moving step stops it,
    :266-272); max_calls (None: none) as the step limit."""
    x0, y0, phi0, xt, yt = start
    c = reference_episode_config(start=(float(x0), float(y0), float(phi0), 0.0, 0.0),
                                 target=(float(xt), float(yt)), max_steps=max_calls or 0,
                                 enumerate=True)
    c.p_turn_right = c.p_turn_left = c.p_new_target = 0
    c.stop_rule = 1
    return c
