"""Causal rectangular attention cases (udm_attention_fwd_kv_causal: query i sees the keys j <= i + (Lk - Lq)) shared by tests/test_attention_kv_causal_ref64.py
(CPU) and tests/test_gpu_attention_kv_causal_rowwise.py (GPU): the families of tests/attention_ref64.py built at L = Lk, the first Lq rows as the queries.

The shapes: offset 0 ((1, 1), (5, 5), (130, 130): the square case, the last with a second query tile) and offsets that are no multiple of 64; one query row
((1, 1), (1, 200): it sees every key); the frontier inside the ragged last key tile ((77, 333), (129, 193), (200, 264), (48, 560)); a second query tile whose
walk ends at another key tile than the first one's ((129, 193): tiles [0, 3) and [0, 4); (130, 130): [0, 2) and [0, 3); (200, 264): [0, 3) and [0, 5))."""
import attention_ref64 as R

SHAPES = ((1, 1), (1, 200), (5, 5), (64, 128), (77, 333), (129, 193), (130, 130), (48, 560), (200, 264))     # (Lq, Lk)
MUTANT_SHAPES = ((64, 128), (77, 333), (129, 193))      # Lq > 1 and Lk > Lq: where every mask mutant of the CPU module must show
HEAD_DIMS = (32, 64, 128, 256)
FAMILIES = ("gauss", "ramp_up", "row_offset", "spikes", "pointer")


def make_case(family, B, H, Lq, Lk, D, *, prescaled, seed=None):
    """q [B, H, Lq, D], k, v [B, H, Lk, D] (bf16)"""
    q, k, v, _ = R.make_inputs(family, B, H, Lk, D, prescaled=prescaled, seed=Lq + Lk + D if seed is None else seed)
    return q[:, :, :Lq].contiguous(), k, v
