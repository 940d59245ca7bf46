"""Scan policy: the TRUE height scan -- the block of the privileged observation the critic already reads -- as one more input segment of the
HIM actor, from the rollout to the PPO update.

    runner = ScanOnPolicyRunner(env, train_cfg, device=dev)
    runner.enable_graphs()
    runner.learn(n)

This is the privileged teacher of vision distillation (learn/distill.py): a policy that sees the terrain around it exactly, which no robot
does, trained so that a camera student can be regressed onto its action means.  What a map policy does with the elevation map's rows
(learn/map_policy.py), this does with a column slice of the live privileged observation: the same VisionActorCritic with depth_latent_dim =
LSIM_NUM_HEIGHT_PTS, the same storage and the same fused launch, whose extra segment takes a row pitch (lsim_policy_extra.ld =
num_priv_obs), so NO launch and no buffer is added -- the rows are what the critic's blocks of the same launch stage anyway.  There is no
sensor, no encoder and no auxiliary loss, and a HIM policy warm-starts it through load_him_state_dict.  One rank only."""
from .. import abi
from ..envs.sensors import FOOT_CHANNELS, FootScan, TerrainFootScan
from .vision import ActorRowsPPO, ActorRowsRunner, height_scan_block


class ScanPPO(ActorRowsPPO):
    """act() records `latent_source()` (the runner passes the scan block of env.privileged_obs_buf, a column-slice view) with the
    transition, so storage.depth_latent[t] is storage.privileged_observations[t][:, off:off + w] bit for bit, and the update binds each
    minibatch's stored rows to the actor.  update() returns HIMPPO.update()'s tuple."""


class ScanOnPolicyRunner(ActorRowsRunner):
    """HIMOnPolicyRunner for a scan policy.  The env's config needs terrain.measure_heights (height_scan_block raises without it: the
    block would hold zeros).  train_cfg is HIMOnPolicyRunner's; policy["depth_latent_dim"] is set here.  The first actor layer reads
    45 + 3 + 16 + 187 = 251 columns, inside the fused policy launch's 272.
    `foot_scan` (a FootScan) with `channels` = ("foot_height",) (the default then) or ("foot_height", "foot_known"): the privileged teacher
    on TRUE foot scans -- the runner adds a sensors.TerrainFootScan to the env as env.sensors["foot_scan"] (or takes the one that is
    there) and the actor reads its rows, channels * 4K columns, in place of the height scan; the record gains "foot_scan" and "channels"
    and its offset is None.  Without `foot_scan` the runner is exactly what it was.  Distillation from such a teacher is not built."""

    policy_kind = "scan"
    sensor = None           # VisionRollout's: the rows come from the env, not from a sensor

    def __init__(self, env, train_cfg, log_dir=None, device="cpu", fast=None, foot_scan=None, channels=None):
        self.foot_scan, self.channels = foot_scan, None
        if foot_scan is not None:
            return self._init_foot_scan(env, train_cfg, foot_scan, FOOT_CHANNELS[0] if channels is None else tuple(channels), log_dir, device, fast)
        if channels is not None:
            raise ValueError("ScanOnPolicyRunner: channels belongs to foot_scan=FootScan(...)")
        off, width = height_scan_block(env.cfg)
        if env.num_privileged_obs is None or env.num_privileged_obs < off + width:
            raise ValueError(f"ScanOnPolicyRunner: the env's privileged observation has {env.num_privileged_obs} columns, the height scan is [{off}, {off + width})")
        if width != abi.DEFINES["LSIM_NUM_HEIGHT_PTS"]:
            raise ValueError(f"ScanOnPolicyRunner: the height scan has {width} points, the layout {abi.DEFINES['LSIM_NUM_HEIGHT_PTS']}")
        self._check_first_layer(env, **{"scan points": width})
        self.scan = (off, width)
        super().__init__(env, self._rows_cfg(train_cfg, ScanPPO, width), log_dir=log_dir, device=device, fast=fast)
        self.alg.latent_source = lambda: env.privileged_obs_buf[:, off:off + width]

    def _init_foot_scan(self, env, train_cfg, foot_scan, channels, log_dir, device, fast):
        if not isinstance(foot_scan, FootScan):
            raise TypeError(f"ScanOnPolicyRunner: foot_scan is a FootScan, got {type(foot_scan).__name__}")
        if channels not in FOOT_CHANNELS:
            raise ValueError(f"ScanOnPolicyRunner: channels is ('foot_height',) or ('foot_height', 'foot_known'), got {channels}")
        width = len(channels) * 4 * foot_scan.num_points
        self._check_first_layer(env, **{"foot rows": width})
        feet = env.sensors.get("foot_scan")
        if feet is None:
            feet = env.add_sensor("foot_scan", TerrainFootScan(env, foot_scan, channels))
        elif not isinstance(feet, TerrainFootScan) or feet.foot_scan != foot_scan or feet.channels != channels:
            raise ValueError("ScanOnPolicyRunner: env.sensors['foot_scan'] exists and is not a TerrainFootScan of this foot_scan and these channels")
        self.channels, self.scan, self.feet = channels, (None, width), feet
        super().__init__(env, self._rows_cfg(train_cfg, ScanPPO, width), log_dir=log_dir, device=device, fast=fast)
        self.alg.latent_source = feet.rows

    def load_him_state_dict(self, sd):
        """warm start from a HIM policy: the scan columns of the first actor layer are zero (VisionActorCritic.load_him_state_dict)"""
        return self.alg.actor_critic.load_him_state_dict(sd)

    def policy_record(self):
        """the checkpoint's record, and what learn/policy_io.py reads of a runner: learn/evaluate.py and learn/distill.py find the rows from it"""
        if self.foot_scan is not None:
            return {"offset": None, "width": int(self.scan[1]), "dim": int(self.alg.actor_critic.depth_latent_dim), "foot_scan": self.foot_scan.record(),
                    "channels": list(self.channels)}
        return {"offset": int(self.scan[0]), "width": int(self.scan[1]), "dim": int(self.alg.actor_critic.depth_latent_dim)}
