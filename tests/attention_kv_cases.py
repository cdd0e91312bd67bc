"""Rectangular attention cases (Lq queries against Lk keys) shared by tests/test_attention_kv_ref64.py (CPU) and tests/test_gpu_attention_kv_rowwise.py (GPU):
the families of tests/attention_ref64.py built at L = Lk, with the first Lq rows as the queries (the kernel is bidirectional)."""
import attention_ref64 as R

SHAPES = ((48, 560), (77, 333), (129, 193), (8, 72), (128, 640))     # (Lq, Lk) of the GPU module
SHAPES_CPU = SHAPES + ((200, 264),)
HEAD_DIMS = (32, 64, 128, 256)
FAMILIES = ("gauss", "ramp_up", "ramp_down", "row_offset", "spikes", "pointer")


def make_case(family, B, H, Lq, Lk, D, *, prescaled, seed=None):
    """q [B, H, Lq, D], k, v [B, H, Lk, D] (bf16)"""
    q, k, v, _ = R.make_inputs(family, B, H, Lk, D, prescaled=prescaled, seed=Lq + Lk + D if seed is None else seed)
    return q[:, :, :Lq].contiguous(), k, v
