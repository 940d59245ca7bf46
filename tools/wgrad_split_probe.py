"""lsim_k_linear_wgrad_split on the update's two largest hidden layers: lsim_linear_elu_wgrad of the in-tree library with the bf16-pipe form off and
on (tools/wgrad_split_time.py is the same over more shapes, with a JSON record).  python tools/wgrad_split_probe.py"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = {0: "fp32 pipe (off)", 1: "bf16 pipe, split (on)"}


def run():
    import torch
    from isaacgymloco_amd import lib
    B_ = 102400
    L = lib.load()
    for k_in, n_out in ((512, 256), (256, 128)):
        x = torch.randn(B_, k_in, device="cuda:0"); g = torch.randn(B_, n_out, device="cuda:0")
        z = torch.nn.functional.elu(torch.randn(B_, n_out, device="cuda:0"))
        for k in NAMES:
            was = L.lsim_wgrad_split_bf16(k)
            need, parts = ctypes.c_size_t(), ctypes.c_int()
            lib.check(L.lsim_linear_wgrad_workspace(B_, k_in, n_out, ctypes.byref(need), ctypes.byref(parts)))
            ws = torch.empty(need.value // 4, device="cuda:0")
            dw, db, gy = torch.empty(n_out, k_in, device="cuda:0"), torch.empty(n_out, device="cuda:0"), torch.empty(B_, n_out, device="cuda:0")
            s = torch.cuda.current_stream().cuda_stream

            def call():
                lib.check(L.lsim_linear_elu_wgrad(x.data_ptr(), k_in, g.data_ptr(), n_out, z.data_ptr(), n_out, B_, k_in, n_out, dw.data_ptr(), db.data_ptr(),
                                                  gy.data_ptr(), ws.data_ptr(), need.value, s))
            for _ in range(5):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(30):
                call()
            e1.record(); torch.cuda.synchronize()
            print(f"{k_in}->{n_out}  {NAMES[k]:32s} {e0.elapsed_time(e1) * 1000 / 30:8.1f} us (incl. the partial-sum launch)")
            L.lsim_wgrad_split_bf16(was)


if __name__ == "__main__":
    run()
