"""TEST INFRASTRUCTURE -- the scenes of the fused elevation-map launch, shared by the CPU tests (the shim) and the GPU tests (the library).
All are dyadic, N = 3 (lifecycle: 4, every third), G = 16, R = 8, six captures each: res = 2^-4, a camera that looks straight down from z = 1 with the identity pose, depths multiples of 2^-10, so every point,
zmax and df * 65536 are exact and sum and count are integers the reference shares; the floats are compared under the reference's bound.

Rays: 0..4 fall into the robot's own cell A (5 points: above count_cap = 4), 5..6 two cells further in x (2 points), 7 four cells further
in y (1 point).  `run(make_rig, name, mutant)` drives the scene's captures and returns (the worst miss in units of the bound, the last
read): at most 1 for the header's rules, and above 10 for the mutant the scene is there to catch (elevation_fuse_reference.MUTANTS)."""
import numpy as np

import elevation_fuse_reference as FR
import elevation_map_reference as ER

F = np.float32
RES, Q = 2.0 ** -4, 2.0 ** -6
DIRS = np.array([[0, 0, -1]] * 5 + [[0.25, 0, -1]] * 2 + [[0, 0.5, -1]], F)
PTS = np.array([[0, 0], [0.125, 0], [0, 0.25], [0.5, 0.5], [-0.125, 0]], F)
POSE = (0.5 + 2 * Q, 0.25 + 2 * Q, 1.0)          # the centre of its cell
k8 = lambda *k: F(0.5) + np.array(k, F) * F(2.0 ** -8)

# name -> (fusion, [(tick, flags, depths [8], pose or None, episode_length or None)], N, env_stride, exact ties)
SCENES = {
    # cell A: df = 0, 2^-7, 2^-6 inside the band 2^-4, then 0.125 and 0.25 outside it
    "spread": ({}, [(3, 0, k8(0, 2, 4, 32, 64, 0, 1, 0), None, None), (4, 0, k8(1, 3, 5, 33, 65, 2, 3, 1), None, None),
                    (5, 0, k8(4, 2, 0, 64, 32, 1, 0, 0), None, None), (6, 0, k8(2, 2, 5, 40, 50, 3, 3, 1), None, None),
                    (7, 0, k8(1, 2, 3, 30, 31, 0, 2, 0), None, None), (8, 0, k8(0, 2, 4, 32, 64, 0, 1, 0), None, None)], 3, 1, False),
    # cell A holds 5 points within the band (cap 4 reached), the others 2 and 1 (not reached)
    "counts": ({}, [(3, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (8, 0, k8(1, 1, 2, 3, 5, 1, 1, 1), None, None),
                    (9, 0, k8(0, 2, 2, 3, 4, 0, 2, 0), None, None), (12, 0, k8(1, 1, 3, 3, 5, 1, 1, 1), None, None),
                    (13, 0, k8(0, 1, 2, 4, 4, 0, 1, 0), None, None), (20, 0, k8(1, 1, 2, 3, 5, 1, 1, 1), None, None)], 3, 1, False),
    # 1000 ticks between the captures: the prior's variance has grown by 2^-20 * 1000, twenty times the measurement's
    "ageing": ({"var_growth": 2.0 ** -20}, [(10, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (1010, 0, k8(1, 2, 3, 4, 5, 1, 2, 1), None, None),
                                            (1015, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (3015, 0, k8(1, 1, 2, 3, 4, 1, 1, 1), None, None),
                                            (3016, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (9016, 0, k8(1, 2, 3, 4, 5, 1, 2, 1), None, None)], 3, 1, False),
    # first write, fuse, a step of +5/32 m and back: the gate opens twice and the newest capture wins
    "steps": ({}, [(1, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (2, 0, k8(1, 1, 2, 3, 4, 0, 1, 1), None, None),
                   (3, 0, k8(*(np.array([0, 1, 2, 3, 4, 0, 1, 0]) - 40)), None, None), (4, 0, k8(*(np.array([1, 1, 2, 3, 4, 1, 1, 0]) - 40)), None, None),
                   (5, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (6, 0, k8(1, 2, 2, 3, 4, 0, 1, 1), None, None)], 3, 1, False),
    # sigma = 2^-5, vm = 2^-10, S = 2^-9, d = 2^-4 in the one-point cell: d^2 == gate2 S exactly, and the strict gate stays shut
    "gate_edge": ({"sigma0": 2.0 ** -5, "sigma2": 0.0, "var_floor": 0.0, "var_growth": 0.0, "var_max": 1.0, "gate2": 2.0, "count_cap": 1, "band": 0.0},
                  [(1, 0, k8(0, 0, 0, 0, 0, 0, 0, 0), None, None), (2, 0, k8(-16, -16, -16, -16, -16, -16, -16, -16), None, None)] +
                  [(3 + k, 0, k8(*([-16 * (k % 2)] * 8)), None, None) for k in range(4)], 3, 1, True),
    # vm is about 5e-5: above var_max = 3e-5 at the first write, and K vm falls below var_floor = 2.5e-5 at the first fusion
    "clamps": ({"var_max": 3e-5}, [(1, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (2, 0, k8(1, 1, 2, 3, 4, 0, 1, 1), None, None),
                                   (3, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (4, 0, k8(1, 1, 2, 3, 4, 0, 1, 1), None, None),
                                   (5, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (6, 0, k8(1, 1, 2, 3, 4, 0, 1, 1), None, None)], 3, 1, False),
    # stamps 0x7FFFFFFE: five ticks later the tick's low word is 0x80000003, then (a new episode) 3 -- the age is 5 both times
    "wrap": ({"var_growth": 2.0 ** -20}, [(2 ** 31 - 2, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (2 ** 31 + 3, 0, k8(1, 1, 2, 3, 4, 0, 1, 1), None, None),
                                          (2 ** 32 - 2, ER.FILL_ALL, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (2 ** 32 + 3, 0, k8(1, 1, 2, 3, 4, 0, 1, 1), None, None),
                                          (2 ** 32 + 4, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (2 ** 32 + 9, 0, k8(1, 1, 2, 3, 4, 0, 1, 1), None, None)], 3, 1, False),
    # N = 4, every third env: fill, a capture, the window scrolls 20 cells away and back, env 0 starts an episode, RESETS_ONLY with env 3 reset
    "lifecycle": ({}, [(0, ER.FILL_ALL, k8(0, 1, 2, 3, 4, 0, 1, 0), None, None), (1, 0, k8(1, 1, 2, 3, 4, 0, 1, 1), None, None),
                       (2, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), (POSE[0] + 20 * RES, POSE[1], 1.0), None), (3, 0, k8(2, 1, 2, 3, 4, 0, 1, 1), POSE, None),
                       (4, 0, k8(0, 1, 2, 3, 4, 0, 1, 0), None, (0, 1, 1, 1)), (5, ER.RESETS_ONLY, k8(3, 1, 2, 3, 4, 0, 1, 1), None, (1, 1, 1, 0))], 4, 3, False),
}
CATCHES = {"no_growth": "ageing", "K_swapped": "ageing", "gate_inclusive": "gate_edge", "no_gate": "steps", "no_clamp": "clamps", "no_cap": "counts",
           "no_wrap": "wrap", "band_on_z": "spread", "sum_all": "spread"}
assert set(CATCHES) == set(FR.MUTANTS)


def run(make_rig, name, mutant=None, reverse=False, G=16, stream=None, repeat=False):
    fusion, captures, N, stride, ties = SCENES[name]
    order = slice(None, None, -1) if reverse else slice(None)
    rig = make_rig(N, G, DIRS[order], PTS, fusion=fusion, res=RES, env_stride=stride, unknown_drop=0.5)
    ref = FR.RefFused(N, ER.Params.of(rig), rig.read(), fusion)
    ref.exact_ties = ties
    rs = rig.get("root_states")
    shift = np.arange(N, dtype=F)[:, None] * np.array([4 * RES, -2 * RES, 0.0], F)        # every env in a cell of its own, the same rays
    rs[:, :3] = np.array(POSE, F) + shift
    rig.put("root_states", rs)
    worst, reads = 0.0, []
    for tick, flags, depths, pose, el in captures:
        if pose is not None:
            rs[:, :3] = np.array(pose, F) + shift
            rig.put("root_states", rs)
        rig.put("episode_length", np.ones(N, np.int64) if el is None else np.array(el, np.int64))
        rig.put("depth", np.broadcast_to(depths[order], (N, 8)).copy())
        assert rig.launch(tick, flags, stream=stream) == 0
        got = rig.read()
        ref.step(rig.inputs(), tick, flags, mutant)
        worst = max(worst, FR.worst_miss(got, ref))
        reads.append(got)
    return worst, reads, ref
