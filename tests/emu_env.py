"""TEST INFRASTRUCTURE -- the product's LeggedRobot Python surface (isaacgymloco_amd/envs/legged_robot.py: the class a user of the reference
switches to) with the CPU lane emulator of the kernel sources (tests/emu, tests/emu_binding.py) in place of the HIP library, so that code
which only exists in the build container -- the REFERENCE's own runner classes -- can drive that surface end to end without a GPU.
Everything above the C-ABI is the product's code unchanged: constructor, buffer binding, step() / reset() / reset_idx(), extras, the
attribute names runners read.  Nothing under isaacgymloco_amd/ imports this module."""
import emu_binding
from isaacgymloco_amd.envs.legged_robot import LeggedRobot


class EmuLeggedRobot(LeggedRobot):
    def __init__(self, cfg, sim_params=None, physics_engine=None, sim_device="cpu", headless=True, **kw):
        super().__init__(cfg, sim_params, physics_engine, "cpu", headless, **kw)

    def _load_library(self):
        return emu_binding.EmuApi(emu_binding.lib())      # every entry point LeggedRobot calls, lsim_create_mixed included

    def _sync(self):
        pass

    def _stream(self):
        return None
