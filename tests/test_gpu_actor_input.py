"""GPU: lsim_actor_input (csrc/ls_learn.h) -- the general kernel, which no other test launches ((45, 16) takes the 64-lane one) -- against the
fp64 reference: the copied columns bit for bit, the normalised latent within 4 x the distance of the reference's fp32 twins; row strides wider
than the rows with NaN in the unused columns; one row whose latent is all zeros gives 0, not NaN."""
import numpy as np
import pytest
import torch

import mlp_shapes_reference as R
import mlp_shapes_rig as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("batch", R.ACTOR_INPUT_BATCHES)
@pytest.mark.parametrize("n1,latent", R.ACTOR_INPUT_CASES)
def test_actor_input_matches_the_reference(n1, latent, batch):
    from isaacgymloco_amd import lib
    L = lib.load()
    obs, enc, ref, tol = G.actor_input_scene(n1, latent, batch)
    o, e = torch.from_numpy(obs).to(G.DEV), torch.from_numpy(enc).to(G.DEV)
    W = n1 + 3 + latent
    out, flat = G.guarded((batch, W))
    assert L.lsim_actor_input(o.data_ptr(), o.stride(0), n1, e.data_ptr(), e.stride(0), latent, batch, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert G.guards_intact(flat, batch * W)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :n1], obs[:, :n1]) and np.array_equal(got[:, n1:n1 + 3], enc[:, :3])
    err = float(np.abs(got[:, n1 + 3:].astype(np.float64) - ref[:, n1 + 3:]).max())
    print((n1, latent, batch), "max |device - fp64|", err, "tolerance", tol)
    assert np.isfinite(got).all() and err <= tol
    if batch > 1:
        assert not got[batch // 2, n1 + 3:].any()
