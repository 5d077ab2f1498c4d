"""What the per-pixel losses (flow.py, depth.py) share on the host: the kinds, the tiling of ex4dgs_amd/csrc/ex4d_pixel_stream.h, and the
checks and allocations around a forward and a backward call.  `name` is the rendered tensor's name as the messages carry it
("out_flow", "out_depth"), `what` the loss's ("flow", "depth")."""
import torch

KINDS = {"l1": 0, "charbonnier": 1}           # EX4D_FLOW_L1 / EX4D_DEPTH_L1, EX4D_FLOW_CHARBONNIER / EX4D_DEPTH_CHARBONNIER
PIXELS_PER_LANE, THREADS, FOLD = 4, 256, 64   # EX4D_FLOW_* and EX4D_DEPTH_* _PIXELS_PER_LANE, _THREADS, _FOLD
CODE_DTYPES = (torch.uint16, torch.int16)     # 16-bit codes: the same bits in either


def kind_code(kind):
    if kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r}: one of {sorted(KINDS)}")
    return KINDS[kind]


def require_device(rendered, name, what):
    if not rendered.is_cuda:
        raise RuntimeError(f"{name} is on {rendered.device}: the {what} loss kernels only run on a ROCm GPU (no CPU fallback)")


def check_acc(acc, H, W, dev, name):
    if acc is not None and (acc.dtype != torch.float32 or acc.numel() != H * W or acc.device != dev or not acc.is_contiguous()):
        raise RuntimeError(f"acc must be a contiguous float32 [H,W] or [1,H,W] tensor on {name}'s device")


def check_row(row, n, dev, name):
    if row.dtype != torch.float64 or row.device != dev or row.numel() != n or not row.is_contiguous():
        raise RuntimeError(f"row must be a contiguous float64 [{n}] tensor on {name}'s device")


def check_grad_loss(grad_loss, dev, name):
    if grad_loss.dtype != torch.float32 or grad_loss.device != dev or grad_loss.numel() != 1:
        raise RuntimeError(f"grad_loss must be a float32 tensor of one element on {name}'s device")


def forward_outputs(loss, row, scratch, n_row, need, scratch_dtype, unit, dev, name):
    """(loss float32 [1], row float64 [n_row], scratch of `need` elements of scratch_dtype): each allocated when absent, checked when given."""
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    if row is None:
        row = torch.empty(n_row, dtype=torch.float64, device=dev)
    else:
        check_row(row, n_row, dev, name)
    if scratch is None:
        scratch = torch.empty(need, dtype=scratch_dtype, device=dev)
    elif scratch.dtype != scratch_dtype or scratch.device != dev or scratch.numel() < need or not scratch.is_contiguous():
        raise RuntimeError(f"scratch must be a contiguous {str(scratch_dtype)[6:]} tensor of at least {need} {unit} on {name}'s device")
    return loss, row, scratch


def gradient_output(out, rendered, fits, shape, name):
    """The backward's output: a new tensor like `rendered`, or `out` where it is float32, contiguous, on the device and fits(out)."""
    if out is None:
        return torch.empty_like(rendered)
    if out.dtype != torch.float32 or out.device != rendered.device or not fits(out) or not out.is_contiguous():
        raise RuntimeError(f"out must be a contiguous float32 {shape} tensor on {name}'s device")
    return out
