"""Map policy: the elevation map's scan (envs/sensors.py, ElevationMap) as one more input segment of the HIM actor, from the rollout to the
PPO update.

    cam = env.add_sensor("depth", depth_camera(env, 64, 48, 87.0, model=SensorModel(period=5, stagger=True)))
    cam.attach_map(ElevationMap(size=32), odometry=OdometryError(scale=0.02, yaw_per_m=0.01, z_per_m=0.01))
    runner = MapOnPolicyRunner(env, train_cfg, sensor="depth", channels=("height", "known"), device=dev)
    runner.enable_graphs()
    runner.learn(n)

What a vision policy does with the depth encoder's latent (learn/vision.py), this does with the rows lsim_map_rows builds from the map --
the heights around the robot in the units of the privileged height scan, and optionally which of them the map knows: the same
VisionActorCritic with depth_latent_dim = channels * P, the same storage and the same fused launch carry "some [N, dim] rows behind the
latent" from the rollout to the update, and a HIM policy warm-starts it through load_him_state_dict.  There is no encoder, no auxiliary loss
and no snapshot: the rows are the map's, and no gradient goes anywhere but into the actor-critic.  One rank only."""
from ..envs.sensors import FOOT_CHANNELS, FootScan
from .vision import ActorRowsPPO, ActorRowsRunner

CHANNELS = (("height",), ("height", "known"), ("height", "confidence")) + FOOT_CHANNELS


class MapPPO(ActorRowsPPO):
    """act() records `latent_source()` (the runner passes sensor.map_rows) with the transition and the update binds each minibatch's
    stored rows to the actor; there is no encoder, so no snapshots are kept and no encoder or memory step follows.  update() returns
    HIMPPO.update()'s tuple."""


class MapOnPolicyRunner(ActorRowsRunner):
    """HIMOnPolicyRunner for a map policy.  `sensor`: the name of a sensor already added to the env (env.add_sensor), or the sensor; it needs
    an attached ElevationMap (cam.attach_map, with or without odometry).  `channels`: ("height",), ("height", "known") or, for a map with a
    fusion, ("height", "confidence") -- how far each height can be trusted, lsim_map_rows_fused, under the width rule of two channels; the runner calls
    cam.attach_map_rows(channels) and the actor reads cam.map_rows(), channels * P more columns.  train_cfg is HIMOnPolicyRunner's;
    policy["depth_latent_dim"] is set here.  The fused policy launch takes a first actor layer of at most 272 columns: 187 points with
    one channel (251 columns), and with two channels a map of at most 104 points (ElevationMap(points=...), e.g. 11 x 9).
    `channels` = ("foot_height",) or ("foot_height", "foot_known") with `foot_scan` (a FootScan; None: its defaults): the actor reads the
    map at a small pattern around each foot instead (lsim_foot_scan, cam.attach_map_rows(channels, foot_scan=...)), channels * 4K columns:
    the default K = 25 gives 100 or 200 (264 columns with two channels), and one channel takes at most K = 52.  Whether foot scans help
    on stairs has not been trained long enough to say."""

    policy_kind = "map"

    def __init__(self, env, train_cfg, sensor="depth", channels=("height",), log_dir=None, device="cpu", fast=None, foot_scan=None):
        cam = env.sensors[sensor] if isinstance(sensor, str) else sensor
        if getattr(cam, "map", None) is None:
            raise ValueError("MapOnPolicyRunner: the sensor has no elevation map (cam.attach_map(ElevationMap(...)))")
        channels = tuple(channels)
        if channels not in CHANNELS:
            raise ValueError(f"MapOnPolicyRunner: channels is ('height',), ('height', 'known'), ('height', 'confidence'), ('foot_height',) or "
                             f"('foot_height', 'foot_known'), got {channels}")
        feet = channels in FOOT_CHANNELS
        if foot_scan is not None and not feet:
            raise ValueError(f"MapOnPolicyRunner: foot_scan belongs to the foot channels, got channels {channels}")
        if feet:
            foot_scan = FootScan() if foot_scan is None else foot_scan
            if not isinstance(foot_scan, FootScan):
                raise TypeError(f"MapOnPolicyRunner: foot_scan is a FootScan, got {type(foot_scan).__name__}")
        if channels[-1] == "confidence" and getattr(cam.map, "fusion", None) is None:
            raise ValueError("MapOnPolicyRunner: the channel 'confidence' needs a map with a fusion (ElevationMap(fusion=MapFusion(...)))")
        dim = len(channels) * (4 * foot_scan.num_points if feet else int(cam.map_scan().shape[1]))       # the width of the rows to come
        self._check_first_layer(env, **{"foot rows" if feet else "map rows": dim})
        self.sensor, self.channels = cam, channels
        super().__init__(env, self._rows_cfg(train_cfg, MapPPO, dim), log_dir=log_dir, device=device, fast=fast)
        cam.attach_map_rows(channels, foot_scan=foot_scan)       # behind the parent's env.reset(): the sensor has captured, so every env's rows are built now
        self.alg.latent_source = cam.map_rows

    def policy_record(self):
        cam = self.sensor                   # what the policy was trained with: learn/evaluate.py rebuilds sensor, map, odometry and rows from it
        return {"sensor": cam.spec() if hasattr(cam, "spec") else None, "channels": list(self.channels), "dim": int(self.alg.actor_critic.depth_latent_dim)}
