"""GPU: the whole chain once on the device -- a 64 x 48 see-robot camera with an instrument error, the stereo artefacts, a noisy-source
elevation map and the depth encoder on a full LeggedRobot on stairs -- for a fill, three steps and a reset_idx.  The reference is computed
from the DEVICE's own out, label and instrument rows and the history a twin sensor without the option leaves (given the camera's history
before every capture, on the same env, seed, tick and stream), all read back: the device's ray cast need not match the CPU build's bit for
bit, so nothing here compares across the two."""
import numpy as np
import pytest
import torch

import sensor_stereo_emu_binding as B
import sensor_stereo_reference as REF
from test_gpu_elevation_map_chain import DEV, _camera, _env

pytestmark = pytest.mark.gpu
N, W, H = 16, 64, 48


def test_the_chain_on_the_device_matches_the_reference_on_its_own_rows():
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    env = _env(5, num_envs=N)
    model = sensors.SensorModel(period=2, stagger=True, latency=2, frames=2, noise=(0.01, 0.002), dropout=0.02, normalise=True)
    inst = sensors.InstrumentError(latency=(0, 2), noise_gain=(0.5, 2.0), depth_scale=0.02, fov=0.02)
    stereo = sensors.StereoArtifacts()
    cam = _camera(env, see_robot=True, labels=True, model=model, instrument=inst, stereo=stereo)
    twin = _camera(env, see_robot=True, labels=True, model=model, instrument=inst)
    torch.manual_seed(3)
    enc = DepthEncoder(H, W, 2).to(DEV)
    cam.attach_encoder(enc)
    cam.attach_map(sensors.ElevationMap(size=32, source="noisy"))
    assert cam.chain() == ("lsim_sensor_instrument", "lsim_sensor_capture_inst", "lsim_sensor_stereo", "lsim_elevation_map", "lsim_depth_encode")
    st = cam.stage("stereo").struct
    p = {k: getattr(st, k) for k in B.SCALARS}
    inv_scale = (1.0 / cam.scale).cpu().numpy()
    state = np.zeros(2, np.int64)
    g = torch.Generator().manual_seed(2)
    for step in range(5):
        if step == 0:
            tick, flags = 0, REF.FILL_ALL
        elif step == 3:
            env.reset_idx([2, 5, 11])
            tick, flags = int(env.common_step_counter), REF.RESETS_ONLY
        else:
            env.step_device((torch.randn(N, 12, generator=g) * 0.3).to(DEV))
            tick, flags = int(env.common_step_counter), 0
        twin.history().copy_(cam.history())
        cam.update(tick=tick, flags=flags)
        twin.update(tick=tick, flags=flags)
        torch.cuda.synchronize()
        assert bool((cam.out == twin.out).all()) and bool((cam.instrument_rows() == twin.instrument_rows()).all())
        hist, state, codes = REF.apply(twin.history().cpu().numpy()[:, :, :W * H], state, cam.out.cpu().numpy(), cam.labels().cpu().numpy(), inv_scale,
                                       env.episode_length_buf.cpu().numpy(), cam.instrument_rows().cpu().numpy(), p, tick, flags)
        got = cam.history().cpu().numpy()[:, :, :W * H]
        assert (got.view(np.uint32) == hist.view(np.uint32)).all(), f"step {step}: {int((got.view(np.uint32) != hist.view(np.uint32)).sum())} elements differ"
        assert cam.stereo_counts().tolist() == state.tolist(), f"step {step}"
        print(f"step {step}: due {int((codes != 0).any(axis=1).sum())} envs, holes {int((codes == REF.HOLE).sum())}, fattened {int((codes == REF.FATTEN).sum())}")
    assert state[0] > 0 and state[1] > 0
    for name, t in (("frames", cam.frames()), ("latent", cam.latent()), ("scan", cam.map_scan()), ("out", cam.out), ("rows", cam.instrument_rows())):
        assert bool(torch.isfinite(t).all()), name
    assert int(cam.nonfinite_rays) == 0 and int(cam.map_nonfinite) == 0
