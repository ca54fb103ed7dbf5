"""What the GPU test files of the training step share: a hand-made or fixture batch as the dict `Engine.train_step` takes from the
sampler, and the chain kernel's per-point record read back from the workspace."""
import numpy as np
import torch


def smp(b, max_rays=None):
    """batch dict (pc, z_vals, depth_sample, dirs_C_sample, dirs_W_sample, norm_sample, indices_b / _h / _w, n_frames) -> the
    sampler-shaped dict on the device.  max_rays: the arrays already hold that many ray slots, of which `b["n_valid"]` are live."""
    d = lambda a: torch.as_tensor(a).cuda()
    R, S = b["z_vals"].shape
    n_valid = R if max_rays is None else int(b["n_valid"])
    return dict(n_valid=torch.tensor([n_valid], dtype=torch.int32, device="cuda"), pc=d(b["pc"]), z_vals=d(b["z_vals"]),
                depth_sample=d(b["depth_sample"]), dirs_C_sample=d(b["dirs_C_sample"]), dirs_W_sample=d(b["dirs_W_sample"]),
                norm_sample=None if b["norm_sample"] is None else d(b["norm_sample"]), indices_b=d(b["indices_b"]),
                indices_h=d(b["indices_h"]), indices_w=d(b["indices_w"]), max_rays=R, S=S, n_frames=b["n_frames"])


def pe_aux(eng, N):
    """the chain kernel's per-point record for the dW kernel, read back from the workspace: [x' (3), 0, gbar' (3), s_G] ([N, 8]).
    Offset as make_workspace (isdf_common.h) lays it out: the last region before the 256 + 4 096 spare bytes."""
    import ctypes as C
    total = int(eng.lib.isdf_workspace_bytes(C.byref(eng.cnet), N, 1))
    nbytes = -(-N // 64) * 64 * 32
    off = total - 256 - 4096 - nbytes
    return eng._ws[off:off + nbytes].view(torch.float32).view(-1, 8)[:N].cpu().numpy().astype(np.float64)
