"""ctypes binding of the in-tree native library (csrc/ -> libdrynx_native.so).

Every op takes torch tensors.  If the tensors live on a GPU the gfx950 kernel
is launched on torch's current HIP stream; otherwise the same functor runs on
the host thread pool inside the library.  There is no pure-Python fallback for
any op: if the library is missing the import fails loudly (and on a GPU box the
driver can see exactly which .so was loaded).

Tensor conventions (all int32 tensors carrying raw u32 limbs, little endian):
  Fp / scalar : [..., 8]
  G1 affine   : [..., 16]   (x, y) Montgomery, infinity = zeros
  G1 Jacobian : [..., 24]
  G2 affine   : [..., 32]
  Fp12 (GT)   : [..., 96]
"""
from __future__ import annotations

import collections
import ctypes
import os
import threading

import numpy as np

import torch

from .. import kmeans as km
from .. import rounds

_HERE = os.path.dirname(os.path.abspath(__file__))
# DRYNX_NATIVE_LIB selects another build of the library (e.g. the host-sanitizer
# build, build/libdrynx_native_asan.so); default: the in-tree gfx950 build
LIB_PATH = os.environ.get("DRYNX_NATIVE_LIB") or os.path.join(_HERE, "libdrynx_native.so")

_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if os.environ.get("DRYNX_AUTOBUILD", "1") == "1":
            from . import build as _b

            _b.build()
        else:
            raise ImportError(f"{LIB_PATH} missing: run `python -m drynx_amd.native.build`")
    _lib = ctypes.CDLL(LIB_PATH)
    _declare(_lib)
    return _lib


_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_int64

_SIGS = {
    "dx_fp_to_mont": [_I, _P, _P, _P, _L],
    "dx_fp_from_mont": [_I, _P, _P, _P, _L],
    "dx_field_probe": [_I, _P, _I, _P, _P, _P, _L],
    "dx_fr_arith": [_I, _P, _I, _P, _P, _P, _L, _L],
    "dx_fr_dot_chunks": [_I, _P, _P, _P, _I, _P, _L, _L, _L],
    "dx_fr_seg_sum": [_I, _P, _P, _P, _P, _L],
    "dx_rp_challenges": [_I, _P, _P, _P, _P, _P, _P, _L],
    "dx_g1_fb_table": [_I, _P, _P, _P, _P, _L],
    "dx_g1_fb_mul": [_I, _P, _P, _P, _P, _L],
    "dx_g1_fb_mul_i64": [_I, _P, _P, _P, _P, _L],
    "dx_g1_fb_mul_idx": [_I, _P, _P, _P, _P, _P, _L],
    "dx_g1_mul": [_I, _P, _P, _P, _P, _L, _I, _I],
    "dx_g1_add": [_I, _P, _P, _P, _P, _L, _I, _I],
    "dx_g1_to_affine": [_I, _P, _P, _P, _L],
    "dx_g1_from_affine": [_I, _P, _P, _P, _L],
    "dx_g1_eq": [_I, _P, _P, _P, _P, _L],
    "dx_g1_on_curve": [_I, _P, _P, _P, _L],
    "dx_g1_sum_chunks": [_I, _P, _P, _P, _L, _L, _L],
    "dx_elgamal_encrypt": [_I, _P, _P, _P, _P, _P, _P, _P, _L],
    "dx_bsgs_build": [_I, _P, _P, _L, _P, _P, _L],
    "dx_bsgs_solve": [_I, _P, _P, _P, _P, _P, _L, _L, _L, _L, _P, _P, _L],
    "dx_g2_fb_table": [_I, _P, _P, _P, _P, _L],
    "dx_g2_fb_mul": [_I, _P, _P, _P, _P, _P, _L],
    "dx_g2_mul": [_I, _P, _P, _P, _P, _L, _I],
    "dx_g2_on_curve": [_I, _P, _P, _P, _L],
    "dx_miller_loop": [_I, _P, _P, _P, _P, _L],
    "dx_final_exp": [_I, _P, _P, _P, _L],
    "dx_pairing": [_I, _P, _P, _P, _P, _L],
    "dx_gt_mul": [_I, _P, _P, _P, _P, _L],
    "dx_gt_inv": [_I, _P, _P, _P, _L],
    "dx_prg_glv": [_I, _P, _P, ctypes.c_uint32, _P, _P, _P, _L],
    "dx_prg_bits": [_I, _P, _P, ctypes.c_uint32, _I, _P, _L],
    "dx_batched_copy": [_I, _P, _P, _P, _I, _L],
    "dx_copy_out": [_I, _P, _P, _P, _I, _L, _I],
    "dx_host_device_ptr": [_P, _P],
    "dx_rows_all": [_I, _P, _P, _P, _I, _L, _P],
    "dx_gt_pow": [_I, _P, _P, _P, _P, _L, _I],
    "dx_gt_eq": [_I, _P, _P, _P, _P, _L],
    "dx_gt_fb_table": [_I, _P, _P, _P, _P, _L],
    "dx_gt_fb_pow": [_I, _P, _P, _P, _P, _P, _L],
    "dx_gt_prod_chunks": [_I, _P, _P, _P, _L, _L, _L],
    "dx_version": [],
    "dx_lr_moments": [_P, _P, _P, _L, _I, _P, _I, _I],
    "dx_lr_gd_k2": [_P, _P, _P, _I, ctypes.c_double, ctypes.c_double, ctypes.c_double, _I, ctypes.c_double,
                    ctypes.c_double, ctypes.c_double, _P],
    "dx_random_scalars": [_I, _P, _P, ctypes.c_uint32, _P, _L],
    "dx_sha256_chunks": [_I, _P, _P, _L, _L, _P],
    "dx_hash_to_g1": [_I, _P, _P, _P, _L, _P, _L],
    "dx_lr_encode": [_P, _P, _L, _L, _I, _P, _P, _P, _L, _I, ctypes.c_double, ctypes.c_double, _P, _L, _I, _I, _P, _P,
                     _L, _I],
    "dx_lr_reduce": [_P, _P, _L, _L, _L, _P],
    "dx_lr_reduce_pack": [_P, _P, _L, _I, _I, _I, _L, ctypes.c_double, _P, _P],
    "dx_g1_mul_glv256": [_P, _P, _P, _P, _P, _L, _I, _I, _I],
    "dx_glv_split": [_I, _P, _P, _P, _L],
    "dx_gt_t2_compress": [_I, _P, _P, _P, _P, _L],
    "dx_g2_x_compress": [_I, _P, _P, _P, _P, _P, _L],
    "dx_g2_x_decompress": [_I, _P, _P, _P, _P, _P, _L],
    "dx_gt_t2_decompress": [_I, _P, _P, _P, _L],
    "dx_gt_slice_prod": [_I, _P, _P, _P, _P, _P, _P, _L],
    "dx_gt_chunk_weight": [_I, _P, _P, _P, _P, _P, _P, _P, _L],
    "dx_gt_beta_rows": [_I, _P, _P, _P, _L, _L],
    "dx_gt_beta_slice_prod": [_I, _P, _P, _P, _P, _P, _P, _L],
    "dx_gt_pi": [_I, _P, _P, _P, _L],
    "dx_g1_mul_glv": [_P, _P, _P, _P, _P, _L, _I],
    "dx_rp_u_joint_split": [_I, _P, _P, _P, _P, _L, _I, _I, _L, _I, _P, _P],
    "dx_bucket_bounds": [_I, _P, _P, _L, _L, _P, _P],
    "dx_slice_desc": [_I, _P, _P, _P, _P, _I, _L, _L, _P, _P],
    "dx_lane_slices": [_I, _P, _P, _P, _P, _P, _P, _L, _P, _P],
    "dx_g1_slice_sum": [_I, _P, _P, _P, _P, _P, _P, _L],
    "dx_rp_prove_a": [_I, _P, _P, _P, _P, _P, _P, _L, _I, _I],
    "dx_rp_prove_a_tab": [_I, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I],
    "dx_g2_fb4_table": [_I, _P, _P, _P, _P, _L],
    "dx_g2_fb4_mul": [_I, _P, _P, _P, _P, _P, _L],
    "dx_gt_fb4_table": [_I, _P, _P, _P, _P, _L],
    "dx_gt_fb4_pow": [_I, _P, _P, _P, _P, _P, _L],
    "dx_gt_cyclotomic": [_I, _P, _P, _P, _L],
    "dx_gt_membership": [_I, _P, _P, _P, _L],
    "dx_g1_horner_host": [_P, _P, _L, _I, _I],
    "dx_fp_sqrt_host": [_P, _P, _P, _P, _L],
    "dx_g2_chunk_weight": [_I, _P, _P, _P, _P, _P, _P, _P, _L],
    "dx_g2_subgroup": [_I, _P, _P, _P, _L],
    "dx_limbs_canonical": [_I, _P, _P, _I, _P, _L],
    "dx_g1j_on_curve": [_I, _P, _P, _P, _L],
    "dx_fold_steps": [],
    "dx_rp_coeffs": [_P, _P, _P, _L],
    "dx_int_moments": [_I, _P, _P, _L, _I, _P, _L, _P, _I, _P, _P],
    "dx_iter_round": [_I, _P, _P, _L, _P, _L, _P, _L, _I, _L, _L, _L, _L, _L, _P, _P],
    "dx_iter_round_cells": [_I, _P, _P, _L, _I, _L, _P, _L, _P, _I, _P, _I, _L, _L, _L, _L, _P, _L, _L, _P],
    "dx_iter_round_cells_pred": [_I, _P, _P, _L, _I, _L, _P, _L, _P, _I, _P, _I, _L, _L, _L, _L, _P, _L, _L, _P, _P],
    "dx_iter_round_max_counters": [],
    "dx_group_moments": [_I, _P, _P, _L, _I, _P, _L, _I, _P, _L, _P, _I, _P, _I, _P, _I, _L, _L, _P],
    "dx_group_moments_pred": [_I, _P, _P, _L, _I, _P, _L, _I, _P, _L, _P, _I, _P, _I, _P, _I, _L, _L, _P, _P],
    "dx_group_moments_max_cells": [],
    "dx_group_cells": [_I, _P, _P, _L, _I, _L, _P, _I, _P, _I, _P],
    "dx_kmeans_round": [_I, _P, _P, _L, _P, _L, _L, _P, _L, _L, _L, _L, _L, _P],
    "dx_kmeans_max_cells": [],
    "dx_group_cells_pred": [_I, _P, _P, _L, _I, _L, _P, _I, _P, _I, _P, _P],
    "dx_sha256_rows": [_I, _P, _P, _L, _L, _L, _L, _P],
    "dx_sha256_segments": [_I, _P, _P, _L, _L, _L, _P],
    "dx_g1_aff_to_uv": [_I, _P, _P, _L],
    "dx_rp_ncoeffs": [_P, _P, _P, _P, _L],
    "dx_rp_accum_n": [_P, _P, _P, _P, _P, _L, _L, _I, _I],
    "dx_ufold_coop_raw": [_P, _P, _P, _P, _P, _L, _L, _L],
    "dx_gt_frob8": [_I, _P, _P, _P, _L],
    "dx_g2_joint_table": [_I, _P, _P, _P, _L],
    "dx_g2_joint_table_signed": [_I, _P, _P, _P, _P, _L],
    "dx_rp_u_group": [_I, _P, _P, _P, _P, _P, _P, _P, _L, _I, _L, _I, _I, _L, _P, _P],
    "dx_rp_u_joint": [_I, _P, _P, _P, _P, _L, _I, _I, _L, _P],
    "dx_g2_slice_sum": [_I, _P, _P, _P, _P, _P, _P, _L, _I, _L],
    "dx_g2_horner": [_I, _P, _P, _P, _I, _I, _I, _L, _L],
    "dx_rp_msm_uv": [_I, _P, _P, _P, _L, _I, _L],
    "dx_msm_keys": [_I, _P, _P, _P, _L, _L, _I, _I, _P, _P],
    "dx_gls8_entries": [],
    "dx_g2_gls8_table": [_I, _P, _P, _P, _P, _L],
    "dx_gt_gls8_table": [_I, _P, _P, _P, _P, _L, _P, _L],
    "dx_g2_gls8_mul": [_I, _P, _P, _P, _P, _P, _L],
    "dx_rp_prove_a_gls8": [_I, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _P],
    "dx_gt16_entries": [],
    "dx_gt16_table": [_I, _P, _P, _P, _P],
}


def _declare(lib):
    for name, args in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int


def lib():
    return _load()


def loaded_path() -> str:
    _load()
    return LIB_PATH


# ----------------------------------------------------------------------------- helpers
_keep = threading.local()


def _ptr(t: torch.Tensor | None, strided: bool = False):
    """Raw pointer of a contiguous tensor for a native call.  The tensor is
    kept alive until the calling thread's next ``_call`` returns: a temporary
    such as ``_ptr(x.contiguous())`` would otherwise be freed before the call
    runs (on the host path the native code would then read freed memory).
    ``strided``: the op takes the tensor's strides itself."""
    if t is None:
        return None
    assert strided or t.is_contiguous(), "native ops need contiguous tensors"
    held = getattr(_keep, "held", None)
    if held is None:
        held = _keep.held = []
    held.append(t)
    return ctypes.c_void_p(t.data_ptr())


def _ctx(*ts):
    dev = None
    for t in ts:
        if t is not None:
            dev = t.device
            break
    for t in ts:
        if t is not None and t.device != dev:
            raise ValueError(f"native op mixes devices {dev} and {t.device}")
    if dev is not None and dev.type == "cuda":
        if _CHECK_DEVICE and torch.cuda.current_device() != dev.index:
            # DRYNX_CHECK_DEVICE=1 (the GPU suite): a thread launching on a GPU
            # that is not its current device was never pinned to the rank's
            raise AssertionError(f"native op on {dev} from a thread whose current device is "
                                 f"cuda:{torch.cuda.current_device()}")
        return 1, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    return 0, None


_CHECK_DEVICE = os.environ.get("DRYNX_CHECK_DEVICE", "0") == "1"


def _raw_call(name, *args) -> int:
    """A native call whose return code the caller interprets; releases the
    tensors ``_ptr`` held for it, like ``_call``."""
    try:
        return getattr(_load(), name)(*args)
    finally:
        _keep.held = []


def _call(name, *args):
    rc = _raw_call(name, *args)
    if rc != 0:
        raise RuntimeError(f"native op {name} failed (rc={rc})")


def _rows(t: torch.Tensor, width: int) -> int:
    assert t.dtype == torch.int32 and t.shape[-1] == width, (t.dtype, t.shape, width)
    return t.numel() // width


# ----------------------------------------------------------------------------- field
def fp_to_mont(x: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(x)
    g, s = _ctx(x)
    _call("dx_fp_to_mont", g, s, _ptr(x), _ptr(out), _rows(x, 8))
    return out


def fp_from_mont(x: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(x)
    g, s = _ctx(x)
    _call("dx_fp_from_mont", g, s, _ptr(x), _ptr(out), _rows(x, 8))
    return out


PROBE_FP_MUL, PROBE_FP_SQR, PROBE_FR_MUL, PROBE_FP2_MUL, PROBE_FP2_SQR, PROBE_FP2_MUL_FP = range(6)


def field_probe(opc: int, a: torch.Tensor, b: torch.Tensor | None = None) -> torch.Tensor:
    """Raw Montgomery products of the field core, row by row (tests only):
    out = a * b * 2^-256 mod the modulus on the limbs as given.  Rows are 8
    words (Fp, Fr) or 16 (Fp2); PROBE_FP2_MUL_FP takes a [n, 16] and b [n, 8];
    the squarings ignore b."""
    wa = 16 if opc >= PROBE_FP2_MUL else 8
    wb = 8 if opc == PROBE_FP2_MUL_FP else wa
    n = _rows(a, wa)
    if opc in (PROBE_FP_SQR, PROBE_FP2_SQR):
        b = a
    else:
        assert _rows(b, wb) == n, (a.shape, b.shape)
    out = torch.empty_like(a)
    g, s = _ctx(a, b)
    _call("dx_field_probe", g, s, opc, _ptr(a), _ptr(b), _ptr(out), n)
    return out


FR_ADD, FR_SUB, FR_MUL, FR_NEG, FR_INV, FR_REDUCE = range(6)


def fr_arith(op: int, a: torch.Tensor, b: torch.Tensor | None = None) -> torch.Tensor:
    """Row-wise Fr op of a [n, 8] with b: n rows, or k rows read periodically
    (row i uses b[i % k]; k = 1 broadcasts one scalar), canonical in and out."""
    n = _rows(a, 8)
    out = torch.empty_like(a)
    bb = b.contiguous() if b is not None else None
    nb = _rows(bb, 8) if bb is not None else 0
    bcast = nb if (bb is not None and nb != n) else 0
    assert bcast == 0 or n % nb == 0, (n, nb)
    g, s = _ctx(a, bb)
    _call("dx_fr_arith", g, s, op, _ptr(a), _ptr(bb), _ptr(out), n, bcast)
    return out


def fr_dot_rows(a: torch.Tensor, b: torch.Tensor | None, groups: int, b_periodic: bool = False,
                chunk: int = 32) -> torch.Tensor:
    """Per-group Fr sums of a[g*m + k] * b(g, k) -> [groups, 8] (canonical).
    b: None (plain sums), [groups*m, 8] (per row) or [m, 8] (b_periodic)."""
    n = _rows(a, 8)
    m = n // groups
    assert m * groups == n and m > 0
    if b is not None:
        assert _rows(b, 8) == (m if b_periodic else n)
    cur, bb = a.contiguous(), None if b is None else b.contiguous()
    while True:
        n_chunks = (m + chunk - 1) // chunk
        out = torch.empty((groups * n_chunks, 8), dtype=torch.int32, device=a.device)
        g, s = _ctx(cur, bb)
        _call("dx_fr_dot_chunks", g, s, _ptr(cur), _ptr(bb), int(b_periodic), _ptr(out), groups, m, chunk)
        cur, bb, m = out, None, n_chunks
        if m == 1:
            return cur


def fr_seg_sum(a: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """Per-segment Fr sums of the rows of a: out[t] = sum a[offs[t]:offs[t+1]]
    (canonical; offs int64 [k+1] on a's device, non-decreasing, <= rows)."""
    k = offs.numel() - 1
    assert k >= 0 and offs.dtype == torch.int64
    out = torch.empty((k, 8), dtype=torch.int32, device=a.device)
    if k:
        offs = offs.to(a.device).contiguous()
        g, s = _ctx(a, offs, out)
        _call("dx_fr_seg_sum", g, s, _ptr(a.contiguous()), _ptr(offs), _ptr(out), k)
    return out

# ----------------------------------------------------------------------------- G1
def g1_fb_table(base_aff: torch.Tensor) -> torch.Tensor:
    """Comb table(s) [n_bases*8192, 16] for one or more affine G1 bases."""
    bases = base_aff.contiguous().view(-1, 16)
    nb = bases.shape[0]
    table = torch.empty((nb * 8192, 16), dtype=torch.int32, device=base_aff.device)
    work = torch.empty((nb * 256, 24), dtype=torch.int32, device=base_aff.device)
    g, s = _ctx(bases)
    _call("dx_g1_fb_table", g, s, _ptr(bases), _ptr(work), _ptr(table), nb)
    return table


def g1_fb_mul(table: torch.Tensor, scalars: torch.Tensor) -> torch.Tensor:
    n = _rows(scalars, 8)
    out = torch.empty((n, 24), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(table, scalars)
    _call("dx_g1_fb_mul", g, s, _ptr(table), _ptr(scalars), _ptr(out), n)
    return out


def g1_fb_mul_idx(tables: torch.Tensor, tab_idx: torch.Tensor, scalars: torch.Tensor) -> torch.Tensor:
    """k_i * base_{tab_idx[i]} over stacked comb tables [n_bases*8192, 16]."""
    n = _rows(scalars, 8)
    assert tab_idx.dtype == torch.int32 and tab_idx.numel() == n
    out = torch.empty((n, 24), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(tables, tab_idx, scalars)
    _call("dx_g1_fb_mul_idx", g, s, _ptr(tables), _ptr(tab_idx), _ptr(scalars), _ptr(out), n)
    return out


def g1_fb_mul_i64(table: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    assert m.dtype == torch.int64
    n = m.numel()
    out = torch.empty((n, 24), dtype=torch.int32, device=m.device)
    g, s = _ctx(table, m)
    _call("dx_g1_fb_mul_i64", g, s, _ptr(table), _ptr(m.contiguous()), _ptr(out), n)
    return out


# rows up to which g1_mul runs two lanes per row (the latency form; tools/bench_g1mul.py)
G1_MUL_PAIR_ROWS = 1 << 14


def gt_t2_compress(a: torch.Tensor, out: torch.Tensor | None = None):
    """GT elements [n, 96] -> (c [n, 48] int32, ok [n] uint8): c = (1 + g) / h
    of f = g + h w (torus T2; csrc/kernels/dx_gt_t2.hip); ok = 1 where the
    decompression gives back exactly these limbs (canonical, unitary, h != 0).
    ``out``: a contiguous [n, 48] destination for c; then only ok is returned."""
    n = _rows(a, 96)
    c = torch.empty((n, 48), dtype=torch.int32, device=a.device) if out is None else out
    assert c.is_contiguous() and _rows(c, 48) == n
    ok = torch.empty((n,), dtype=torch.uint8, device=a.device)
    g, s = _ctx(a, c)
    _call("dx_gt_t2_compress", g, s, _ptr(a.contiguous()), _ptr(c), _ptr(ok), n)
    return ok if out is not None else (c, ok)


def gt_t2_decompress(c: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """[n, 48] torus-compressed GT elements -> [n, 96] (``out``: a contiguous
    destination of that shape, e.g. a slice of a payload being rebuilt)."""
    n = _rows(c, 48)
    out = torch.empty((n, 96), dtype=torch.int32, device=c.device) if out is None else out
    assert out.is_contiguous() and _rows(out, 96) == n
    g, s = _ctx(c, out)
    _call("dx_gt_t2_decompress", g, s, _ptr(c.contiguous()), _ptr(out), n)
    return out


def g2_x_compress(V: torch.Tensor, x_out: torch.Tensor | None = None, flag_out: torch.Tensor | None = None):
    """Affine G2 [n, 32] -> (x [n, 16], flag [n] int32: y parity | 2 * infinity,
    ok [n] uint8: canonical and on the twist, i.e. ``g2_x_decompress`` gives the
    same limbs back).  ``x_out`` / ``flag_out``: contiguous destinations."""
    n = _rows(V, 32)
    x = torch.empty((n, 16), dtype=torch.int32, device=V.device) if x_out is None else x_out
    f = torch.empty((n,), dtype=torch.int32, device=V.device) if flag_out is None else flag_out
    assert x.is_contiguous() and f.is_contiguous() and x.numel() == 16 * n and f.numel() == n
    ok = torch.empty((n,), dtype=torch.uint8, device=V.device)
    g, s = _ctx(V, x, f)
    _call("dx_g2_x_compress", g, s, _ptr(V.contiguous()), _ptr(x), _ptr(f), _ptr(ok), n)
    return x, f, ok


def g2_x_decompress(x: torch.Tensor, flag: torch.Tensor, out: torch.Tensor | None = None):
    """(x [n, 16], flag [n]) -> (affine G2 [n, 32], bad [n] uint8: no point
    with that x)."""
    n = _rows(x, 16)
    V = torch.empty((n, 32), dtype=torch.int32, device=x.device) if out is None else out
    assert V.is_contiguous() and V.numel() == 32 * n and flag.numel() == n
    bad = torch.empty((n,), dtype=torch.uint8, device=x.device)
    g, s = _ctx(x, flag, V)
    _call("dx_g2_x_decompress", g, s, _ptr(x.contiguous()), _ptr(flag.contiguous()), _ptr(V), _ptr(bad), n)
    return V, bad


def glv_split(scalars: torch.Tensor) -> torch.Tensor:
    """[n, 8] scalars -> [n, 9] int32 words: k1 (4), |k2| (4), k2 < 0 with
    k = k1 + k2 GLV_LAMBDA mod r (csrc/bn254/glv_split.h; host or device)."""
    n = _rows(scalars, 8)
    out = torch.empty((n, 9), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(scalars)
    _call("dx_glv_split", g, s, _ptr(scalars.contiguous()), _ptr(out), n)
    return out


def g1_mul(pts_jac: torch.Tensor, scalars: torch.Tensor) -> torch.Tensor:
    np_ = _rows(pts_jac, 24)
    nk = _rows(scalars, 8)
    n = max(np_, nk)
    assert np_ in (1, n) and nk in (1, n)
    out = torch.empty((n, 24), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(pts_jac, scalars)
    if g:  # gfx950: in-kernel GLV split, 128-step ladder (dx_g1_varmul.hip)
        rc = _raw_call("dx_g1_mul_glv256", s, _ptr(pts_jac), _ptr(scalars), _ptr(_glv_const("beta", out.device)),
                       _ptr(out), n, int(np_ == 1 and n > 1), int(nk == 1 and n > 1), int(n <= G1_MUL_PAIR_ROWS))
        if rc:
            raise RuntimeError(f"dx_g1_mul_glv256 failed rc={rc}")
        return out
    _call("dx_g1_mul", g, s, _ptr(pts_jac), _ptr(scalars), _ptr(out), n, int(np_ == 1 and n > 1),
          int(nk == 1 and n > 1))
    return out


def g1_add(a: torch.Tensor, b: torch.Tensor, subtract: bool = False) -> torch.Tensor:
    n = _rows(a, 24)
    nb = _rows(b, 24)
    assert nb in (1, n)
    out = torch.empty((n, 24), dtype=torch.int32, device=a.device)
    g, s = _ctx(a, b)
    _call("dx_g1_add", g, s, _ptr(a), _ptr(b), _ptr(out), n, int(subtract), int(nb == 1 and n > 1))
    return out


def g1_to_affine(jac: torch.Tensor) -> torch.Tensor:
    n = _rows(jac, 24)
    out = torch.empty((n, 16), dtype=torch.int32, device=jac.device)
    g, s = _ctx(jac)
    _call("dx_g1_to_affine", g, s, _ptr(jac), _ptr(out), n)
    return out


def g1_from_affine(aff: torch.Tensor) -> torch.Tensor:
    n = _rows(aff, 16)
    out = torch.empty((n, 24), dtype=torch.int32, device=aff.device)
    g, s = _ctx(aff)
    _call("dx_g1_from_affine", g, s, _ptr(aff), _ptr(out), n)
    return out


def g1_eq(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    n = _rows(a, 24)
    assert _rows(b, 24) == n
    out = torch.empty((n,), dtype=torch.uint8, device=a.device)
    g, s = _ctx(a, b)
    _call("dx_g1_eq", g, s, _ptr(a), _ptr(b), _ptr(out), n)
    return out


def g1_on_curve(aff: torch.Tensor) -> torch.Tensor:
    n = _rows(aff, 16)
    out = torch.empty((n,), dtype=torch.uint8, device=aff.device)
    g, s = _ctx(aff)
    _call("dx_g1_on_curve", g, s, _ptr(aff), _ptr(out), n)
    return out


def limbs_canonical(x: torch.Tensor, fr: bool = False) -> torch.Tensor:
    """uint8 per 8-limb row: row < p (Fp, Montgomery coordinates) or < r (Fr)."""
    n = _rows(x, 8)
    out = torch.empty((n,), dtype=torch.uint8, device=x.device)
    g, s = _ctx(x)
    _call("dx_limbs_canonical", g, s, _ptr(x.contiguous()), int(fr), _ptr(out), n)
    return out


def g1j_on_curve(jac: torch.Tensor) -> torch.Tensor:
    n = _rows(jac, 24)
    out = torch.empty((n,), dtype=torch.uint8, device=jac.device)
    g, s = _ctx(jac)
    _call("dx_g1j_on_curve", g, s, _ptr(jac.contiguous()), _ptr(out), n)
    return out


def g2_subgroup(aff: torch.Tensor) -> torch.Tensor:
    """uint8 per affine twist point: on the curve and in G2 (psi(Q) == [6u^2] Q)."""
    n = _rows(aff, 32)
    out = torch.empty((n,), dtype=torch.uint8, device=aff.device)
    g, s = _ctx(aff)
    _call("dx_g2_subgroup", g, s, _ptr(aff.contiguous()), _ptr(out), n)
    return out


def gt_cyclotomic(a: torch.Tensor) -> torch.Tensor:
    """uint8 per Fp12: non-zero and in the cyclotomic subgroup (x^(p^4) x == x^(p^2))."""
    n = _rows(a, 96)
    out = torch.empty((n,), dtype=torch.uint8, device=a.device)
    g, s = _ctx(a)
    _call("dx_gt_cyclotomic", g, s, _ptr(a.contiguous()), _ptr(out), n)
    return out


def gt_membership(a: torch.Tensor) -> torch.Tensor:
    """[n] uint8: a_i in the prime-order GT, for a_i in the cyclotomic subgroup
    (x^p == x^(6u^2): one Frobenius against two cyclotomic u-ladders)."""
    n = _rows(a, 96)
    out = torch.empty((n,), dtype=torch.uint8, device=a.device)
    g, s = _ctx(a)
    _call("dx_gt_membership", g, s, _ptr(a.contiguous()), _ptr(out), n)
    return out


def g1_sum(x: torch.Tensor, chunk: int = 64) -> torch.Tensor:
    """Sum over axis 0 of x[n_items, n_groups, 24] (Jacobian) -> [n_groups, 24].

    Multi-pass chunked reduction: each pass has n_groups * ceil(items/chunk)
    independent threads, so wide vectors and deep reductions both fill the GPU.
    """
    assert x.dim() == 3 and x.shape[-1] == 24
    n_items, n_groups = x.shape[0], x.shape[1]
    cur = x.contiguous()
    if n_items == 0:
        from ..crypto.bn254 import g1_infinity_jac

        return g1_infinity_jac(n_groups, x.device)
    while n_items > 1:
        ch = max(2, min(chunk, n_items)) if n_groups >= 4096 else max(2, min(8, n_items))
        n_chunks = (n_items + ch - 1) // ch
        out = torch.empty((n_chunks, n_groups, 24), dtype=torch.int32, device=x.device)
        g, s = _ctx(cur)
        _call("dx_g1_sum_chunks", g, s, _ptr(cur), _ptr(out), n_items, n_groups, ch)
        cur, n_items = out, n_chunks
    return cur[0]


# ----------------------------------------------------------------------------- ElGamal
def elgamal_encrypt(tabB, tabP, m: torch.Tensor, r: torch.Tensor):
    n = m.numel()
    assert m.dtype == torch.int64 and _rows(r, 8) == n
    K = torch.empty((n, 24), dtype=torch.int32, device=m.device)
    C = torch.empty((n, 24), dtype=torch.int32, device=m.device)
    g, s = _ctx(tabB, tabP, m, r)
    _call("dx_elgamal_encrypt", g, s, _ptr(tabB), _ptr(tabP), _ptr(m.contiguous()), _ptr(r), _ptr(K), _ptr(C), n)
    return K, C


def bsgs_build(tabB: torch.Tensor, m_baby: int, cap: int):
    assert cap & (cap - 1) == 0 and cap >= 2 * m_baby
    keys = torch.zeros((cap,), dtype=torch.int64, device=tabB.device)
    vals = torch.zeros((cap,), dtype=torch.int32, device=tabB.device)
    g, s = _ctx(tabB)
    _call("dx_bsgs_build", g, s, _ptr(tabB), m_baby, _ptr(keys), _ptr(vals), cap)
    return keys, vals


def bsgs_solve(targets_jac, giant_aff, keys, vals, m_baby: int, n_giant: int, offset: int):
    n = _rows(targets_jac, 24)
    out = torch.empty((n,), dtype=torch.int64, device=targets_jac.device)
    found = torch.empty((n,), dtype=torch.uint8, device=targets_jac.device)
    g, s = _ctx(targets_jac, giant_aff, keys, vals)
    _call("dx_bsgs_solve", g, s, _ptr(targets_jac), _ptr(giant_aff), _ptr(keys), _ptr(vals), keys.numel(), m_baby,
          n_giant, offset, _ptr(out), _ptr(found), n)
    return out, found


# ----------------------------------------------------------------------------- G2
def g2_fb_table(base_aff: torch.Tensor) -> torch.Tensor:
    """Comb table(s) [n_bases*8192, 32] for one or more affine G2 bases."""
    bases = base_aff.contiguous().view(-1, 32)
    nb = bases.shape[0]
    table = torch.empty((nb * 8192, 32), dtype=torch.int32, device=base_aff.device)
    work = torch.empty((nb * 256, 48), dtype=torch.int32, device=base_aff.device)
    g, s = _ctx(bases)
    _call("dx_g2_fb_table", g, s, _ptr(bases), _ptr(work), _ptr(table), nb)
    return table


def g2_fb_mul(tables: torch.Tensor, scalars: torch.Tensor, tab_idx: torch.Tensor | None = None) -> torch.Tensor:
    n = _rows(scalars, 8)
    out = torch.empty((n, 32), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(tables, scalars, tab_idx)
    _call("dx_g2_fb_mul", g, s, _ptr(tables), _ptr(tab_idx), _ptr(scalars), _ptr(out), n)
    return out


FB4_ENTRIES = 960  # 64 windows x 15 non-zero digits


def _window_table(sym: str, bases: torch.Tensor, width: int, entries: int, windows: int, work_width: int,
                  out: torch.Tensor | None) -> torch.Tensor:
    """Windowed fixed-base table(s) [n_bases*entries, width] by the native
    builder ``sym`` (``windows`` work rows of ``work_width`` words per base).
    ``out``: a preallocated slice of a larger table tensor to fill in place."""
    assert bases.dtype == torch.int32
    bases = bases.contiguous().view(-1, width)
    nb = bases.shape[0]
    table = out if out is not None else torch.empty((nb * entries, width), dtype=torch.int32, device=bases.device)
    assert table.shape == (nb * entries, width) and table.is_contiguous()
    work = torch.empty((nb * windows, work_width), dtype=torch.int32, device=bases.device)
    g, s = _ctx(bases, table)
    _call(sym, g, s, _ptr(bases), _ptr(work), _ptr(table), nb)
    return table


def g2_fb4_table(base_aff: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """4-bit comb table(s) [n_bases*960, 32] (120 KiB per base)."""
    return _window_table("dx_g2_fb4_table", base_aff, 32, FB4_ENTRIES, 64, 48, out)


def g2_fb4_mul(tables: torch.Tensor, scalars: torch.Tensor, tab_idx: torch.Tensor | None = None) -> torch.Tensor:
    n = _rows(scalars, 8)
    out = torch.empty((n, 32), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(tables, scalars, tab_idx)
    _call("dx_g2_fb4_mul", g, s, _ptr(tables), _ptr(tab_idx), _ptr(scalars), _ptr(out), n)
    return out


GLS8_ENTRIES = 2176  # 17 signed byte windows x 128 digits (csrc/kernels/dx_gls8.hip)


def g2_gls8_table(base_aff: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """GLS-2 signed 8-bit fixed-base table(s) [n_bases*2176, 32] (272 KiB per base)."""
    return _window_table("dx_g2_gls8_table", base_aff, 32, GLS8_ENTRIES, 17, 48, out)


def gt_gls8_table(bases: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """GLS-2 signed 8-bit fixed-base table(s) [n_bases*2176, 48] of GT elements
    as torus images beta = (1 + g) / h (csrc/bn254/gt_torus.h; 408 KiB per
    base).  A base 1 (the set's padding point) gets rows of 0xFFFFFFFF words,
    which the prover skips; a base -1 has no image: the native call fails (rc 2)."""
    bases = bases.contiguous()
    nb = _rows(bases, 96)
    table = out if out is not None else torch.empty((nb * GLS8_ENTRIES, 48), dtype=torch.int32, device=bases.device)
    assert table.shape == (nb * GLS8_ENTRIES, 48) and table.is_contiguous()
    work = torch.empty((nb * 17, 96), dtype=torch.int32, device=bases.device)
    g, s = _ctx(bases, table)
    # GPU path: the Fp12 powers of up to 1024 bases at a time (816 KiB each) before they are normalised
    tb = min(nb, 1024) if g else 0
    tmp = torch.empty((tb * GLS8_ENTRIES + 1, 96), dtype=torch.int32, device=bases.device) if g else None
    _call("dx_gt_gls8_table", g, s, _ptr(bases), _ptr(work), _ptr(table), nb, _ptr(tmp), tb)
    return table


def g2_gls8_mul(tables: torch.Tensor, scalars: torch.Tensor, tab_idx: torch.Tensor | None = None) -> torch.Tensor:
    """k * A (affine) from the signed 8-bit GLS-2 table of A: 34 mixed additions."""
    n = _rows(scalars, 8)
    assert tab_idx is None or (tab_idx.dtype == torch.int32 and tab_idx.numel() == n)
    out = torch.empty((n, 32), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(tables, scalars, tab_idx)
    _call("dx_g2_gls8_mul", g, s, _ptr(tables), _ptr(tab_idx), _ptr(scalars), _ptr(out), n)
    return out


_gt16: dict = {}


def gt16_table(device) -> torch.Tensor:
    """gT with signed 16-bit windows: [17 * 32768, 48], the torus images of
    gT^(d 2^(16w)) (107 MB, built once per device; csrc/kernels/dx_gls8.hip)."""
    key = str(torch.device(device))
    if key not in _gt16:
        from ..crypto import bn254 as _bn
        from ..crypto import oracle as _O

        g = _O.pairing(_O.G1_GEN, _O.G2_GEN)
        pows = []
        for _ in range(17):
            pows.append(g)
            for _ in range(16):
                g = g * g
        pow2 = _bn.gt_tensor(pows, device)
        n = _load().dx_gt16_entries()
        table = torch.empty((n, 48), dtype=torch.int32, device=pow2.device)
        gg, s = _ctx(pow2, table)
        tmp = torch.empty((n + 1, 96), dtype=torch.int32, device=pow2.device) if gg else None
        _call("dx_gt16_table", gg, s, _ptr(pow2), _ptr(table), _ptr(tmp))
        _gt16[key] = table
    return _gt16[key]


def g2_mul(pts_aff: torch.Tensor, scalars: torch.Tensor) -> torch.Tensor:
    n = _rows(scalars, 8)
    np_ = _rows(pts_aff, 32)
    assert np_ in (1, n)
    out = torch.empty((n, 32), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(pts_aff, scalars)
    _call("dx_g2_mul", g, s, _ptr(pts_aff), _ptr(scalars), _ptr(out), n, int(np_ == 1 and n > 1))
    return out


def g2_on_curve(aff: torch.Tensor) -> torch.Tensor:
    n = _rows(aff, 32)
    out = torch.empty((n,), dtype=torch.uint8, device=aff.device)
    g, s = _ctx(aff)
    _call("dx_g2_on_curve", g, s, _ptr(aff), _ptr(out), n)
    return out


# ----------------------------------------------------------------------------- pairing / GT
def miller_loop(P_aff: torch.Tensor, Q_aff: torch.Tensor) -> torch.Tensor:
    n = _rows(P_aff, 16)
    assert _rows(Q_aff, 32) == n
    out = torch.empty((n, 96), dtype=torch.int32, device=P_aff.device)
    g, s = _ctx(P_aff, Q_aff)
    _call("dx_miller_loop", g, s, _ptr(P_aff), _ptr(Q_aff), _ptr(out), n)
    return out


def final_exp(f: torch.Tensor) -> torch.Tensor:
    n = _rows(f, 96)
    out = torch.empty_like(f)
    g, s = _ctx(f)
    _call("dx_final_exp", g, s, _ptr(f), _ptr(out), n)
    return out


def pairing(P_aff: torch.Tensor, Q_aff: torch.Tensor) -> torch.Tensor:
    n = _rows(P_aff, 16)
    assert _rows(Q_aff, 32) == n
    out = torch.empty((n, 96), dtype=torch.int32, device=P_aff.device)
    g, s = _ctx(P_aff, Q_aff)
    _call("dx_pairing", g, s, _ptr(P_aff), _ptr(Q_aff), _ptr(out), n)
    return out


_CHUNK_WORDS = 4096


def batched_copy(pairs: list) -> None:
    """``dst.copy_(src)`` for many (src, dst) pairs of one device in ONE
    launch of 16 KB chunks (csrc/kernels/dx_copy.hip); both contiguous, the
    same byte size, a multiple of 4 bytes."""
    pairs = [(s_, d_) for s_, d_ in pairs if s_.numel()]
    if not pairs:
        return
    dev = pairs[0][1].device
    desc = np.empty((len(pairs), 4), dtype=np.int64)
    c0 = 0
    for i, (s_, d_) in enumerate(pairs):
        nb = s_.numel() * s_.element_size()
        assert s_.is_contiguous() and d_.is_contiguous() and s_.device == dev and d_.device == dev
        assert nb == d_.numel() * d_.element_size() and nb % 4 == 0, (s_.shape, d_.shape)
        w = nb // 4
        desc[i] = (s_.data_ptr(), d_.data_ptr(), w, c0)
        c0 += -(-w // _CHUNK_WORDS)
    ht = torch.from_numpy(desc)
    if dev.type == "cuda":
        no_capture("batched_copy")
    dd = ht.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else ht
    g, st = _ctx(pairs[0][1])
    for s_, d_ in pairs:  # held until the call returns
        _ptr(s_), _ptr(d_)
    _call("dx_batched_copy", g, st, _ptr(dd), _ptr(ht), len(pairs), c0)


COPY_OUT_BLOCKS = 32


def copy_to_host(pairs: list, host_base: torch.Tensor, blocks: int = COPY_OUT_BLOCKS) -> None:
    """``dst.copy_(src)`` for (device src, slice of the pinned host buffer
    ``host_base``) pairs in ONE launch of a ``blocks``-workgroup persistent
    grid on the current stream (csrc/kernels/dx_copy.hip copy_out_kernel):
    PCIe-bound like the runtime's blit copy, but on a few CUs instead of
    thousands of waves beside the compute kernels.  4-byte multiples."""
    pairs = [(s_, d_) for s_, d_ in pairs if s_.numel()]
    if not pairs:
        return
    dev = pairs[0][0].device
    assert dev.type == "cuda" and host_base.is_pinned() and host_base.is_contiguous()
    hb = host_base.data_ptr()
    dbase = ctypes.c_int64(0)
    rc = _load().dx_host_device_ptr(ctypes.c_void_p(hb), ctypes.cast(ctypes.pointer(dbase), ctypes.c_void_p))
    if rc:
        raise RuntimeError("pinned buffer has no device mapping")
    hend = hb + host_base.numel() * host_base.element_size()
    desc = np.empty((len(pairs), 4), dtype=np.int64)
    c0 = 0
    for i, (s_, d_) in enumerate(pairs):
        nb = s_.numel() * s_.element_size()
        assert s_.is_contiguous() and d_.is_contiguous() and s_.device == dev and d_.device.type == "cpu"
        assert nb == d_.numel() * d_.element_size() and nb % 4 == 0 and s_.data_ptr() % 4 == 0
        assert hb <= d_.data_ptr() and d_.data_ptr() + nb <= hend and (d_.data_ptr() - hb) % 4 == 0
        w = nb // 4
        desc[i] = (s_.data_ptr(), dbase.value + (d_.data_ptr() - hb), w, c0)
        c0 += -(-w // _CHUNK_WORDS)
    ht = torch.from_numpy(desc)
    no_capture("copy_to_host")
    dd = ht.pin_memory().to(dev, non_blocking=True)
    st = torch.cuda.current_stream(dev).cuda_stream
    for s_, _ in pairs:
        _ptr(s_)
    _call("dx_copy_out", 1, st, _ptr(dd), _ptr(ht), len(pairs), c0, int(blocks))


def _strided_rows(ts: list):
    """[G, *shape] strided view over G equally shaped contiguous blocks that
    sit at a constant byte step in ONE storage, else None."""
    t0 = ts[0]
    # many small blocks only (thousands of one-record DPs): a few large ones
    # copy faster through the batched 16 KB-chunk kernel
    if len(ts) < 256 or not all(t.is_contiguous() and t.shape == t0.shape and t.dtype == t0.dtype for t in ts):
        return None
    st = t0.untyped_storage().data_ptr()
    if any(t.untyped_storage().data_ptr() != st for t in ts):
        return None
    es = t0.element_size()
    step = ts[1].data_ptr() - t0.data_ptr()
    if step % es or step < t0.numel() * es:
        return None
    p0 = t0.data_ptr()
    if any(t.data_ptr() != p0 + g * step for g, t in enumerate(ts)):
        return None
    return t0.as_strided((len(ts), t0.numel()), (step // es, 1))


def cat_rows(groups: list) -> list:
    """``[torch.cat(g) for g in groups]`` (dim 0) with every copy in ONE
    ``batched_copy`` launch.  A one-tensor group is returned as is (no copy);
    groups whose element bytes are not a multiple of 4 use torch.cat."""
    outs, pairs = [], []
    for g_ in groups:
        if len(g_) == 1:
            outs.append(g_[0])
            continue
        t0 = g_[0]
        if any(t.numel() * t.element_size() % 4 for t in g_):
            outs.append(torch.cat(g_))
            continue
        sv = _strided_rows(g_)
        if sv is not None:
            # equally shaped blocks at a constant stride in one storage (the
            # fields of thousands of one-proof bundles packed as rows of one
            # tensor): ONE strided copy, not one copy descriptor per block
            outs.append(sv.clone(memory_format=torch.contiguous_format).view((-1,) + tuple(t0.shape[1:])))
            continue
        out = torch.empty((sum(t.shape[0] for t in g_),) + tuple(t0.shape[1:]), dtype=t0.dtype, device=t0.device)
        o = 0
        for t in g_:
            assert t.dtype == t0.dtype and tuple(t.shape[1:]) == tuple(t0.shape[1:])
            pairs.append((t.contiguous(), out[o: o + t.shape[0]]))
            o += t.shape[0]
        outs.append(out)
    batched_copy(pairs)
    return outs


def rows_all(flags: list, n: int) -> torch.Tensor:
    """uint8 [n]: row p passes iff every flag array (uint8 / bool, n * k_a
    entries, row-major) is non-zero on its k_a entries of row p -- one
    wavefront per row (csrc/kernels/dx_copy.hip), no bool conversions or
    reductions."""
    fl = [f.reshape(-1).contiguous() for f in flags]
    fl = [f.view(torch.uint8) if f.dtype == torch.bool else f for f in fl]
    assert all(f.dtype == torch.uint8 and f.numel() % max(n, 1) == 0 for f in fl)
    out = torch.empty((n,), dtype=torch.uint8, device=fl[0].device)
    if n == 0:
        return out
    for i in range(0, len(fl), 16):
        part = fl[i: i + 16]
        ptrs = np.asarray([f.data_ptr() for f in part], dtype=np.int64)
        ks = np.asarray([f.numel() // n for f in part], dtype=np.int64)
        g, s = _ctx(out)
        for f in part:
            _ptr(f)
        o = out if i == 0 else torch.empty_like(out)
        _call("dx_rows_all", g, s, ptrs.ctypes.data, ks.ctypes.data, len(part), n, _ptr(o))
        if i:
            out &= o
    return out


def gt_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    n = _rows(a, 96)
    out = torch.empty_like(a)
    g, s = _ctx(a, b)
    _call("dx_gt_mul", g, s, _ptr(a), _ptr(b), _ptr(out), n)
    return out


def gt_inv(a: torch.Tensor) -> torch.Tensor:
    """Row-wise inverse in Fp12*."""
    n = _rows(a, 96)
    out = torch.empty_like(a)
    g, s = _ctx(a)
    _call("dx_gt_inv", g, s, _ptr(a.contiguous()), _ptr(out), n)
    return out


def gt_pow(a: torch.Tensor, scalars: torch.Tensor) -> torch.Tensor:
    n = _rows(scalars, 8)
    na = _rows(a, 96)
    out = torch.empty((n, 96), dtype=torch.int32, device=a.device)
    g, s = _ctx(a, scalars)
    _call("dx_gt_pow", g, s, _ptr(a), _ptr(scalars), _ptr(out), n, int(na == 1 and n > 1))
    return out


def gt_eq(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    n = _rows(a, 96)
    out = torch.empty((n,), dtype=torch.uint8, device=a.device)
    g, s = _ctx(a, b)
    _call("dx_gt_eq", g, s, _ptr(a), _ptr(b), _ptr(out), n)
    return out


def gt_fb_table(bases: torch.Tensor) -> torch.Tensor:
    nb = _rows(bases, 96)
    table = torch.empty((nb * 8192, 96), dtype=torch.int32, device=bases.device)
    work = torch.empty((nb * 256, 96), dtype=torch.int32, device=bases.device)
    g, s = _ctx(bases)
    _call("dx_gt_fb_table", g, s, _ptr(bases.contiguous()), _ptr(work), _ptr(table), nb)
    return table


def gt_fb_pow(tables: torch.Tensor, scalars: torch.Tensor, tab_idx: torch.Tensor | None = None) -> torch.Tensor:
    n = _rows(scalars, 8)
    out = torch.empty((n, 96), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(tables, scalars, tab_idx)
    _call("dx_gt_fb_pow", g, s, _ptr(tables), _ptr(tab_idx), _ptr(scalars), _ptr(out), n)
    return out


def gt_fb4_table(bases: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """4-bit comb table(s) [n_bases*960, 96] (360 KiB per base)."""
    return _window_table("dx_gt_fb4_table", bases, 96, FB4_ENTRIES, 64, 96, out)


def gt_fb4_pow(tables: torch.Tensor, scalars: torch.Tensor, tab_idx: torch.Tensor | None = None) -> torch.Tensor:
    n = _rows(scalars, 8)
    out = torch.empty((n, 96), dtype=torch.int32, device=scalars.device)
    g, s = _ctx(tables, scalars, tab_idx)
    _call("dx_gt_fb4_pow", g, s, _ptr(tables), _ptr(tab_idx), _ptr(scalars), _ptr(out), n)
    return out


def gt_prod(x: torch.Tensor, chunk: int = 16) -> torch.Tensor:
    """Product over axis 0 of x[n_items, n_groups, 96] -> [n_groups, 96]."""
    assert x.dim() == 3 and x.shape[-1] == 96
    n_items, n_groups = x.shape[0], x.shape[1]
    cur = x.contiguous()
    while n_items > 1:
        ch = max(2, min(chunk, n_items))
        n_chunks = (n_items + ch - 1) // ch
        out = torch.empty((n_chunks, n_groups, 96), dtype=torch.int32, device=x.device)
        g, s = _ctx(cur)
        _call("dx_gt_prod_chunks", g, s, _ptr(cur), _ptr(out), n_items, n_groups, ch)
        cur, n_items = out, n_chunks
    return cur[0]


# ----------------------------------------------------------------------------- logistic-regression GEMM (K13)
def lr_gd_k2(a0, S, w0, N: float, lam: float, step: float, max_iter: int, C) -> list:
    """FindMinimumWeights for k = 2 on the host (csrc/kernels/dx_lr.hip
    dx_lr_gd_k2; float64 numpy arrays in, the minimum weights out).  The
    ctypes call releases the GIL for the whole descent."""
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    S = np.ascontiguousarray(S, dtype=np.float64)
    w0 = np.ascontiguousarray(w0, dtype=np.float64)
    d1 = a0.shape[0]
    out = np.empty(d1, dtype=np.float64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _load().dx_lr_gd_k2(p(a0), p(S), p(w0), d1, float(N), float(lam), float(step), int(max_iter), float(C[0]),
                             float(C[1]), float(C[2]), p(out))
    if rc:
        raise RuntimeError(f"dx_lr_gd_k2 failed rc={rc}")
    return out.tolist()


def random_scalars(n: int, device) -> torch.Tensor:
    """n uniform nonzero Fr scalars [n, 8] (plain limbs): ChaCha20 keyed with
    256 fresh bits of os.urandom per call, one block per scalar (dx_hash.hip)."""
    device = torch.device(device)
    out = torch.empty((max(0, n), 8), dtype=torch.int32, device=device)
    if n <= 0:
        return out
    key = np.frombuffer(os.urandom(32), dtype="<u4").copy()
    g, s = _ctx(out)
    _call("dx_random_scalars", g, s, key.ctypes.data_as(ctypes.c_void_p), 0, _ptr(out), n)
    return out


def hash_to_g1(seed: bytes, start: int, n: int, device) -> torch.Tensor:
    """[n, 16] affine G1 points h_start .. h_{start+n-1} derived from a 32-byte
    seed by try-and-increment (dx_hash.hip; unknown discrete logarithms)."""
    from ..crypto import oracle as _O

    device = torch.device(device)
    out = torch.empty((max(0, n), 16), dtype=torch.int32, device=device)
    if n <= 0:
        return out
    sd = np.frombuffer(seed, dtype=">u4").astype("<u4").copy()  # seed words as big-endian message words
    e = np.frombuffer(((_O.P + 1) // 4).to_bytes(32, "little"), dtype="<u4").copy()
    g, s = _ctx(out)
    _call("dx_hash_to_g1", g, s, sd.ctypes.data_as(ctypes.c_void_p), e.ctypes.data_as(ctypes.c_void_p), start,
          _ptr(out), n)
    return out


def fp_sqrt_host(vals: list) -> list:
    """[(sqrt or None)] of Python ints mod p (p = 3 mod 4: a^((p+1)/4)), one
    native host batch."""
    from ..crypto import oracle as _O

    n = len(vals)
    if n == 0:
        return []
    a = np.frombuffer(b"".join((int(v) % _O.P).to_bytes(32, "little") for v in vals), dtype="<u4").copy()
    e = np.frombuffer(((_O.P + 1) // 4).to_bytes(32, "little"), dtype="<u4").copy()
    y = np.empty(8 * n, dtype="<u4")
    ok = np.empty(n, dtype=np.uint8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if _load().dx_fp_sqrt_host(p(a), p(e), p(y), p(ok), n):
        raise RuntimeError("dx_fp_sqrt_host failed")
    yb = y.tobytes()
    return [int.from_bytes(yb[32 * i: 32 * i + 32], "little") if ok[i] else None for i in range(n)]


def prg_scalars(key: bytes, n: int, device) -> torch.Tensor:
    """n Fr scalars from ChaCha20 keyed by a 32-byte ``key`` (deterministic:
    Fiat-Shamir challenge vectors expanded on the device)."""
    device = torch.device(device)
    out = torch.empty((max(0, n), 8), dtype=torch.int32, device=device)
    if n <= 0:
        return out
    k = np.frombuffer(key[:32], dtype="<u4").copy()
    g, s = _ctx(out)
    _call("dx_random_scalars", g, s, k.ctypes.data_as(ctypes.c_void_p), 0, _ptr(out), n)
    return out


def sha256_chunks(data: torch.Tensor, chunk: int) -> torch.Tensor:
    """[k, 8] big-endian SHA-256 words of every `chunk`-byte slice of the raw
    bytes of a contiguous tensor (k = ceil(nbytes / chunk), >= 1)."""
    data = data.contiguous()
    nbytes = data.numel() * data.element_size()
    k = max(1, (nbytes + chunk - 1) // chunk)
    out = torch.empty((k, 8), dtype=torch.int32, device=data.device)
    g, s = _ctx(data)
    _call("dx_sha256_chunks", g, s, _ptr(data), nbytes, chunk, _ptr(out))
    return out


def sha256_segments(tensors: list, chunk: int) -> list:
    """``sha256_chunks`` of many contiguous tensors (same device) in ONE
    launch -> list of [k_i, 8] views of one output tensor."""
    if not tensors:
        return []
    dev = tensors[0].device
    ts = [t.contiguous() for t in tensors]
    nbytes = [t.numel() * t.element_size() for t in ts]
    ks = [max(1, (b + chunk - 1) // chunk) for b in nbytes]
    first = np.concatenate([[0], np.cumsum(ks)[:-1]]).astype(np.int64)
    desc = np.empty((len(ts), 3), dtype=np.int64)
    desc[:, 0] = [t.data_ptr() for t in ts]
    desc[:, 1] = nbytes
    desc[:, 2] = first
    total = int(sum(ks))
    out = torch.empty((total, 8), dtype=torch.int32, device=dev)
    d = _upload(desc, dev)
    g, s = _ctx(out)
    # (the descriptor and any contiguous copies are allocated on this stream:
    # the caching allocator reuses them only behind this launch)
    _call("dx_sha256_segments", g, s, _ptr(d), len(ts), total, chunk, _ptr(out))
    return [out[a: a + k] for a, k in zip(first.tolist(), ks)]


INT_MOMENTS_MAX_COLS = 64


def no_capture(what: str):
    """Host-to-device copies from temporary host buffers must not be recorded
    into a HIP graph (a replay would read freed host memory)."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what}: host upload inside a HIP graph capture")


def _upload(a: np.ndarray, device) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a))
    if torch.device(device).type == "cuda":
        no_capture("upload")
        return t.pin_memory().to(device, non_blocking=True)
    return t


def _tile_plan(counts: np.ndarray, min_rows: int = 64):
    """Host-made tile plan of the segmented reductions: ``([n_tiles, 3] int64
    rows (segment, row0, row1), [G + 1] first tile of every segment)``.  Tiles
    are row ranges of one segment, sized so a big DP spreads over ~2k
    workgroups and each tile still streams >= max(64, ``min_rows``) rows
    (rounded up to a multiple of 64; a segment's last tile may be shorter); a
    segment's tiles are consecutive and an empty segment has none."""
    G = len(counts)
    if G == 0:
        return np.zeros((0, 3), dtype=np.int64), np.zeros(1, dtype=np.int64)
    per_tile = max(int(min_rows), -(-int(counts.sum()) // 2048))
    chunk = max(64, (per_tile + 63) // 64 * 64)
    per = np.maximum(1, -(-counts // chunk)) * (counts > 0)
    seg = np.repeat(np.arange(G, dtype=np.int64), per)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    k = np.arange(len(seg), dtype=np.int64) - np.repeat(first[:-1], per)
    r0 = np.repeat(starts, per) + k * chunk
    r1 = np.minimum(r0 + chunk, np.repeat(starts + counts, per))
    return np.stack([seg, r0, r1], axis=1).reshape(-1, 3).astype(np.int64), first


def int_moments(Z: torch.Tensor, seg_rows, pairs) -> torch.Tensor:
    """K14 (csrc/kernels/dx_moments.hip): exact int64 ``out[g, p] = sum over the
    rows of segment g of Z[i, a_p] * Z[i, b_p]`` (mod 2^64), column index
    ``C = Z.shape[1]`` standing for a constant 1.  ``seg_rows`` are the host-known
    row counts of the consecutive segments (one per DP); ``pairs`` a [P, 2]
    int sequence.  One launch for all segments."""
    assert Z.dtype == torch.int64 and Z.dim() == 2 and Z.stride(1) == 1
    C = Z.shape[1]
    pr = np.asarray(pairs, dtype=np.int16).reshape(-1, 2)
    if C > INT_MOMENTS_MAX_COLS or pr.size == 0 or pr.min() < 0 or pr.max() > C:
        raise ValueError(f"int_moments: {C} columns, pairs out of range")
    counts = np.asarray(seg_rows, dtype=np.int64)
    G, P = len(counts), pr.shape[0]
    if counts.sum() != Z.shape[0]:
        raise ValueError(f"int_moments: segments cover {counts.sum()} rows, Z has {Z.shape[0]}")
    out = torch.zeros((G, P), dtype=torch.int64, device=Z.device)
    plan, _ = _tile_plan(counts)
    n_tiles = len(plan)
    if n_tiles == 0:
        return out
    Zc = Z.contiguous()
    tiles = _upload(plan, Z.device)
    pairs_t = _upload(pr, Z.device)
    g, s = _ctx(Zc)
    partial = None if g else torch.empty((n_tiles, P), dtype=torch.int64)
    _call("dx_int_moments", g, s, _ptr(Zc), Zc.stride(0), C, _ptr(tiles), n_tiles, _ptr(pairs_t), P, _ptr(out),
          _ptr(partial))
    return out


GROUP_MOMENTS_MAX_KEYS = 4
GROUP_MOMENTS_MAX_FILTERS = 8
GROUP_MOMENTS_MAX_GROUPS = 1 << 24
# LDS accumulator cells (group of the window x pair) of one launch: what half a
# CU's 160 KiB leaves beside the staging area (csrc/kernels/dx_group_moments.hip
# kMaxCells, exported as dx_group_moments_max_cells)
GROUP_MOMENTS_MAX_CELLS = 5888
# the operators of a predicate's atoms, in the order of their codes (csrc/kernels/group_terms.h kOpEq ..)
GROUP_OPS = ("==", "!=", "<", "<=", ">", ">=")


def _group_terms(what: str, K, n_rows: int, of: str, keys, filters, bins=None, predicate=None):
    """The checked key and filter terms of a grouped op over the key matrix K
    -> (keys, filters, columns of K, G, pred): at most 4 ``(column, offset,
    cardinality)`` and 8 ``(column, value)``, every column inside K, K int64
    with unit column stride and ``n_rows`` rows (those of ``of``), G = the
    product of the cardinalities at most 2^24.  ``predicate``: None (the rows
    that equal every filter's value) or ``(ops, table)``, one operator of
    ``GROUP_OPS`` per filter -- term f is the atom ``K[i, column_f] ops[f]
    value_f`` -- and the truth table of the formula over the atoms as an int,
    bit ``sum(atom_f << f)`` set where a row passes; pred is then the entries'
    host array, the operator codes and the table's four 64-bit words."""
    keys = [tuple(int(x) for x in k) for k in keys]
    filters = [tuple(int(x) for x in f) for f in filters]
    if len(keys) > GROUP_MOMENTS_MAX_KEYS or any(len(k) != 3 for k in keys):
        raise ValueError(f"{what}: {len(keys)} key columns (at most {GROUP_MOMENTS_MAX_KEYS} triples)")
    if len(filters) > GROUP_MOMENTS_MAX_FILTERS or any(len(f) != 2 for f in filters):
        raise ValueError(f"{what}: {len(filters)} filter terms (at most {GROUP_MOMENTS_MAX_FILTERS} pairs)")
    pred = None
    if predicate is not None:
        ops, table = predicate
        ops, table = list(ops), int(table)
        if not filters:
            raise ValueError(f"{what}: a predicate without filter terms")
        if len(ops) != len(filters):
            raise ValueError(f"{what}: {len(ops)} operators for {len(filters)} filter terms")
        for op in ops:
            if op not in GROUP_OPS:
                raise ValueError(f"{what}: unknown operator {op!r} (one of {' '.join(GROUP_OPS)})")
        if not 0 <= table < 1 << (1 << len(filters)):
            raise ValueError(f"{what}: a truth table outside [0, 2^{1 << len(filters)}) for {len(filters)} atoms")
        words = np.array([(table >> (64 * w)) & ((1 << 64) - 1) for w in range(4)], dtype=np.uint64)
        pred = np.concatenate([np.array([GROUP_OPS.index(op) for op in ops], dtype=np.int64), words.view(np.int64)])
    if bins is not None:
        keys = keys + [tuple(int(x) for x in bins)]
        if len(keys[-1]) != 3:
            raise ValueError(f"{what}: bins is one (column, offset, cardinality)")
    CK = 0
    if K is not None:
        assert K.dtype == torch.int64 and K.dim() == 2 and (K.shape[1] <= 1 or K.stride(1) == 1)
        if K.shape[0] != n_rows:
            raise ValueError(f"{what}: K has {K.shape[0]} rows, {of} has {n_rows}")
        CK = K.shape[1]
    G = 1
    for col, _, card in keys:
        if card < 1 or card > GROUP_MOMENTS_MAX_GROUPS:
            raise ValueError(f"{what}: cardinality {card}")
        G *= card
    if G > GROUP_MOMENTS_MAX_GROUPS:
        raise ValueError(f"{what}: {G} groups (at most {GROUP_MOMENTS_MAX_GROUPS})")
    for col in [k[0] for k in keys] + [f[0] for f in filters]:
        if not 0 <= col < CK:
            raise ValueError(f"{what}: column {col} of a {CK}-column key matrix")
    return keys, filters, CK, G, pred


def _terms_call(name: str, pred, *args) -> int:
    """A grouped entry's return code: ``name`` itself without a predicate, its
    ``_pred`` form with the predicate's host array as one more, last argument."""
    if pred is None:
        return _raw_call(name, *args)
    return _raw_call(name + "_pred", *args, pred.ctypes.data_as(_P))


def group_moments(Z: torch.Tensor, K: torch.Tensor | None, seg_rows, pairs, keys=(), filters=(),
                  bins=None, predicate=None) -> torch.Tensor:
    """K14d (csrc/kernels/dx_group_moments.hip): ``int_moments`` filtered and
    grouped, ``out[dp, g, p] = sum over the rows i of segment dp with where(i)
    and key(i) == g of Z[i, a_p] * Z[i, b_p]`` (mod 2^64) -> [n_dp, G, P] int64.

    Z [rows, C], ``seg_rows`` and ``pairs`` are ``int_moments``' (C may be 0: only
    the constant column, counts).  K [rows, CK] int64 holds the key and filter
    columns and is read in place through its row stride (a view is fine; None
    without keys and filters).  ``keys``: up to 4 ``(column of K, offset,
    cardinality)``; a row's group is the mixed-radix number of ``K[i, column] -
    offset`` over the cardinalities, first key most significant, and a row with
    a digit outside ``[0, cardinality)`` is dropped; G is the product of the
    cardinalities (1 without keys).  ``filters``: up to 8 ``(column of K,
    value)``; a row counts if every one of its columns equals the value.
    ``predicate``: ``(ops, table)``, which turns the filters into the atoms
    ``column ops[f] value`` (``GROUP_OPS``, signed) of a formula given by its
    truth table over the atom bits (``_group_terms``); a row counts if the
    formula holds for it.
    ``bins``: one more, innermost key triple beside the 4 -- the counted column
    (x, QueryMin, R) of a frequency count, whose (group, bin) cells are groups.

    One launch per window of ``GROUP_MOMENTS_MAX_CELLS // P`` consecutive
    groups (the accumulators of a window live in LDS), no torch op and no host
    work per record between the uploads and the output."""
    assert Z.dtype == torch.int64 and Z.dim() == 2 and (Z.shape[1] == 0 or Z.stride(1) == 1)
    C = Z.shape[1]
    pr = np.asarray(pairs, dtype=np.int16).reshape(-1, 2)
    if C > INT_MOMENTS_MAX_COLS or pr.size == 0 or pr.min() < 0 or pr.max() > C:
        raise ValueError(f"group_moments: {C} columns, pairs out of range")
    keys, filters, CK, G, pred = _group_terms("group_moments", K, Z.shape[0], "Z", keys, filters, bins, predicate)
    counts = np.asarray(seg_rows, dtype=np.int64).reshape(-1)
    n_dp, P = len(counts), pr.shape[0]
    if counts.sum() != Z.shape[0] or (n_dp and counts.min() < 0):
        raise ValueError(f"group_moments: segments cover {counts.sum()} rows, Z has {Z.shape[0]}")
    out = torch.zeros((n_dp, G, P), dtype=torch.int64, device=Z.device)
    gw = max(1, GROUP_MOMENTS_MAX_CELLS // P)
    # a tile zeroes and flushes its window's cells: it streams at least as many rows
    plan, _ = _tile_plan(counts, min(min(G, gw) * P, 2048))
    n_tiles = len(plan)
    if n_tiles == 0:
        return out
    Zc = Z if C == 0 else Z.contiguous()
    tiles = _upload(plan, Z.device)
    pairs_t = _upload(pr, Z.device)
    kd = np.ascontiguousarray(np.asarray(keys, dtype=np.int64).reshape(-1))
    fd = np.ascontiguousarray(np.asarray(filters, dtype=np.int64).reshape(-1))
    g, s = _ctx(Zc, K)
    for g0 in range(0, G, gw):
        rc = _terms_call("dx_group_moments", pred, g, s, _ptr(Zc), Zc.stride(0) if C else 0, C,
                         _ptr(K, strided=True), K.stride(0) if CK else 0, CK, _ptr(tiles), n_tiles, _ptr(pairs_t), P,
                         kd.ctypes.data_as(_P), len(keys), fd.ctypes.data_as(_P), len(filters), g0, min(gw, G - g0),
                         _ptr(out))
        if rc == -2:
            raise ValueError("group_moments: the entry refused its arguments")
        if rc != 0:
            raise RuntimeError(f"native op dx_group_moments failed (rc={rc})")
    return out


_ITER_KINDS = {"min": 0, "max": 1, "frequencyCount": 2}


def iter_round(name: str, Z: torch.Tensor, seg_rows, qmin: int, qmax: int, base: int, round: int,
               prefix: int) -> torch.Tensor:
    """K14b / K14c (csrc/kernels/dx_iter_round.hip): the [G, base] int64 rows
    every DP of a batch encrypts in round ``round`` of the iterative ``name``
    query (``min``, ``max`` or ``frequencyCount``, the rounds of a quantile
    search).

    Z [rows, n_in] holds the DPs' records back to back (``seg_rows[g]`` rows for
    DP g; only column 0 is read, through Z's row stride).  With R = qmax - qmin
    + 1 and L the smallest integer with base^L >= R, an offset o = x - qmin
    lies under the prefix iff o div base^(L-round) == prefix, and its digit is
    (o div base^(L-1-round)) mod base (``rounds.iter_round``).  min / max: DP
    g's clamped extreme gives o; under the prefix its value v is that digit,
    otherwise (and for a DP without records) v is neutral: 0 for max, base for
    min.  Row g is the unary encoding of v over [0, base-1]: [i < v] for max,
    [i >= v] for min.  frequencyCount: row g counts DP g's records inside
    [qmin, qmax] under the prefix by digit; records outside the domain are
    dropped.  Two launches for all DPs (tile partials -- extremes, or LDS
    histograms -- then the rows); the tile plan is int_moments', for counts
    with tiles of at least ``base`` rows."""
    assert Z.dtype == torch.int64 and Z.dim() == 2
    qmin, qmax, base, prefix = int(qmin), int(qmax), int(base), int(prefix)
    _, lo = rounds.iter_round(name, qmin, qmax, base, round, prefix)
    counting = name == "frequencyCount"
    counts = np.asarray(seg_rows, dtype=np.int64).reshape(-1)
    G = len(counts)
    if counts.sum() != Z.shape[0] or (G and counts.min() < 0):
        raise ValueError(f"iterative {name}: segments cover {counts.sum()} rows, Z has {Z.shape[0]}")
    if Z.shape[0] and Z.shape[1] < 1:
        raise ValueError(f"iterative {name}: Z has no column")
    out = torch.empty((G, base), dtype=torch.int64, device=Z.device)
    if G == 0:
        return out
    plan, first = _tile_plan(counts, base) if counting else _tile_plan(counts)
    n_tiles = len(plan)
    if counting and n_tiles and int((plan[:, 2] - plan[:, 1]).max()) >= 1 << 31:
        raise ValueError(f"iterative {name}: a tile of 2^31 rows or more")
    # one upload: the tiles, then every DP's tile range
    desc = _upload(np.concatenate([plan.reshape(-1), first]), Z.device)
    partial = torch.empty((max(1, n_tiles), base) if counting else (max(1, n_tiles),), dtype=torch.int64,
                          device=Z.device)
    g, s = _ctx(out)
    # (Z is read in place: a view's row stride is the kernel's ldz)
    _call("dx_iter_round", g, s, _ptr(Z, strided=True), Z.stride(0) if Z.shape[0] > 1 else 1,
          _ptr(desc[: 3 * n_tiles]), n_tiles, _ptr(desc[3 * n_tiles:]), G, _ITER_KINDS[name], qmin, qmax, base, lo,
          prefix, _ptr(partial), _ptr(out))
    return out


def rows_of_counts(name: str, cnt: torch.Tensor) -> torch.Tensor:
    """The rows of a counting operation from the counts ``cnt`` [n_dp, ng, n]
    of its bins, on their device: the one-shot SQL encoder's bins
    (``ops.encoding.batch_values_sql``) and the digits of a grouped iterative
    round (``iter_round_cells``)."""
    if name == "frequencyCount":
        return cnt
    occ = (cnt > 0).to(torch.int64)
    if name == "union":
        return occ
    if name == "inter":
        return 1 - occ
    if name == "min":  # an occupied bin at or below i
        return (occ.cumsum(2) > 0).to(torch.int64)
    if name != "max":
        raise ValueError(f"{name} is not derived from counts")
    return ((occ.flip(2).cumsum(2).flip(2) - occ) > 0).to(torch.int64)  # max: an occupied bin above i


# LDS counters (group of the window x digit) of one launch of the grouped rounds: half a CU's 160 KiB
# (csrc/kernels/dx_iter_round.hip kMaxCounters, exported as dx_iter_round_max_counters)
ITER_ROUND_MAX_COUNTERS = 20480


def iter_round_cells(name: str, K: torch.Tensor, seg_rows, xcol: int, qmin: int, qmax: int, base: int, round: int,
                     prefixes, keys=(), filters=(), predicate=None) -> torch.Tensor:
    """K14e (csrc/kernels/dx_iter_round.hip, dx_iter_round_cells): the [n_dp, G,
    base] int64 rows every DP of a batch encrypts in round ``round`` of G
    simultaneous iterative ``name`` searches, one per cell of a WHERE / GROUP BY.

    K [rows, CK] int64 holds the DPs' record tables back to back (``seg_rows[d]``
    rows for DP d) and is read in place through its row stride; ``keys`` and
    ``filters`` and ``predicate`` are ``group_moments``' (at most 4 keys), G the product of the
    cardinalities, and column ``xcol`` of K is the counted one.  Cell g counts
    the rows of its group (``group_moments``' membership rule, the same
    function) with x inside [qmin, qmax] and (x - qmin) div base^(L-round) ==
    ``prefixes[g]`` by their digit ((x - qmin) div base^(L-1-round)) mod base
    (``rounds.iter_round_cells``; ``len(prefixes) == G``); records outside the
    domain are dropped.  min / max: the unary rows of the first / last occupied
    digit, derived from the counts on the device as ``batch_values_sql`` derives
    the one-shot rows ([an occupied digit at or below i] / [one above i]); a
    cell without a record under its prefix gives the all-zero row.

    One launch per window of ``ITER_ROUND_MAX_COUNTERS // base`` consecutive
    groups (the counters of a window live in LDS), one upload for the plan and
    one for the prefixes, no torch op and no host work per record."""
    assert K.dtype == torch.int64 and K.dim() == 2
    qmin, qmax, base, xcol = int(qmin), int(qmax), int(base), int(xcol)
    what = f"iterative {name} over cells"
    keys, filters, CK, G, pred = _group_terms(what, K, K.shape[0], "K", keys, filters, predicate=predicate)
    prefixes = [int(p) for p in prefixes]
    _, lo = rounds.iter_round_cells(name, qmin, qmax, base, round, prefixes, G)
    if not 0 <= xcol < CK:
        raise ValueError(f"{what}: column {xcol} of a {CK}-column key matrix")
    counts = np.asarray(seg_rows, dtype=np.int64).reshape(-1)
    n_dp = len(counts)
    if counts.sum() != K.shape[0] or (n_dp and counts.min() < 0):
        raise ValueError(f"{what}: segments cover {counts.sum()} rows, K has {K.shape[0]}")
    out = torch.zeros((n_dp, G, base), dtype=torch.int64, device=K.device)
    gw = max(1, ITER_ROUND_MAX_COUNTERS // base)
    # a tile zeroes and flushes its window's counters: it streams at least as many rows
    plan, _ = _tile_plan(counts, min(min(G, gw) * base, 2048))
    n_tiles = len(plan)
    if n_tiles == 0:
        return rows_of_counts(name, out)
    if int((plan[:, 2] - plan[:, 1]).max()) >= 1 << 31:
        raise ValueError(f"{what}: a tile of 2^31 rows or more")
    tiles = _upload(plan, K.device)
    pre = _upload(np.asarray(prefixes, dtype=np.int64), K.device)
    kd = np.ascontiguousarray(np.asarray(keys, dtype=np.int64).reshape(-1))
    fd = np.ascontiguousarray(np.asarray(filters, dtype=np.int64).reshape(-1))
    g, s = _ctx(K)
    for g0 in range(0, G, gw):
        rc = _terms_call("dx_iter_round_cells", pred, g, s, _ptr(K, strided=True), K.stride(0), CK, xcol, _ptr(tiles),
                         n_tiles, kd.ctypes.data_as(_P), len(keys), fd.ctypes.data_as(_P), len(filters), qmin, qmax,
                         base, lo, _ptr(pre), g0, min(gw, G - g0), _ptr(out))
        if rc == -2:
            raise ValueError(f"{what}: the entry refused its arguments")
        if rc != 0:
            raise RuntimeError(f"native op dx_iter_round_cells failed (rc={rc})")
    return rows_of_counts(name, out)


def kmeans_round(Z: torch.Tensor, seg_rows, d: int, k: int, qmin: int, qmax: int, scale: int,
                 centroids) -> torch.Tensor:
    """K14f (csrc/kernels/dx_kmeans.hip): the [n_dp, k * (d + 2)] int64 rows every
    DP of a batch encrypts in one round of a k-means query (``drynx_amd.kmeans``).

    Z [rows, >= d] holds the DPs' records back to back (``seg_rows[g]`` rows for
    DP g; columns 0 .. d-1 are read in place through Z's row stride, a column
    view of a wider table is fine).  A row with a coordinate outside [qmin,
    qmax] is dropped; a kept row with the offsets o_j = x_j - qmin goes to the
    cluster c with the smallest sum_j (scale * o_j - centroids[c * d + j])^2,
    the lowest index among equals; row g is cluster-major [n_c, sum o_0 .. sum
    o_(d-1), sum |o|^2] over DP g's kept rows (``kmeans.round_model``).  One
    launch for all DPs, one upload for the tile plan and the centroids, no torch
    op and no host work per record; the tiles stream at least as many rows as
    they zero and flush cells."""
    assert Z.dtype == torch.int64 and Z.dim() == 2 and (Z.shape[1] <= 1 or Z.stride(1) == 1)
    cen = [int(c) for c in centroids]
    km.check(k, d, qmin, qmax, scale, cen)
    counts = np.asarray(seg_rows, dtype=np.int64).reshape(-1)
    n_dp = len(counts)
    if counts.sum() != Z.shape[0] or (n_dp and counts.min() < 0):
        raise ValueError(f"k-means: segments cover {counts.sum()} rows, Z has {Z.shape[0]}")
    if Z.shape[0] and Z.shape[1] < d:
        raise ValueError(f"k-means: Z has {Z.shape[1]} columns, the query reads {d}")
    cells = k * (d + 2)
    out = torch.zeros((n_dp, cells), dtype=torch.int64, device=Z.device)
    plan, _ = _tile_plan(counts, min(cells, 2048))
    n_tiles = len(plan)
    if n_tiles == 0:
        return out
    if Z.device.type == "cuda":
        no_capture("kmeans_round")
    if qmax == qmin:
        scale = 1  # one value: every offset and every centroid is 0, whatever the scale
    # one upload: the tiles, then the centroids
    desc = _upload(np.concatenate([plan.reshape(-1), np.asarray(cen, dtype=np.int64)]), Z.device)
    g, s = _ctx(Z, out)
    rc = _raw_call("dx_kmeans_round", g, s, _ptr(Z, strided=True), Z.stride(0) if Z.shape[0] > 1 else max(1, d),
                   _ptr(desc[: 3 * n_tiles]), n_tiles, n_dp, _ptr(desc[3 * n_tiles:]), k, d, scale, qmin, qmax,
                   _ptr(out))
    if rc == -2:
        raise ValueError("k-means: the entry refused its arguments")
    if rc != 0:
        raise RuntimeError(f"native op dx_kmeans_round failed (rc={rc})")
    return out


def sha256_rows(data: torch.Tensor, chunk: int) -> torch.Tensor:
    """[rows, k, 8] big-endian SHA-256 words of every `chunk`-byte slice of
    every row of a contiguous 2-D tensor (k = ceil(row bytes / chunk), >= 1)."""
    assert data.dim() == 2 and data.is_contiguous()
    rows = data.shape[0]
    row_bytes = data.shape[1] * data.element_size()
    k = max(1, (row_bytes + chunk - 1) // chunk)
    out = torch.empty((rows, k, 8), dtype=torch.int32, device=data.device)
    g, s = _ctx(data)
    _call("dx_sha256_rows", g, s, _ptr(data), rows, row_bytes, row_bytes, chunk, _ptr(out))
    return out


def _lr_padded(rows: int) -> int:
    """Width P of the kernel's [P, P] output for `rows` live rows (level 2 plus
    the level-1 row): 48 while they fit one 3x3 tile-block, the 16-padded row
    count beyond that (csrc/kernels/dx_lr.hip lr_padded)."""
    nt = (rows + 15) // 16
    return 48 if nt <= 3 else 16 * nt


def lr_moments(X: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """sum_i w_i X_i X_i^T on the fp64-MFMA kernel (GPU tensors only), any
    D = X.shape[1] >= 1."""
    assert X.is_cuda and X.dtype == torch.float64 and X.dim() == 2 and X.shape[1] >= 1 and X.is_contiguous()
    N, D = X.shape
    P = _lr_padded(D)
    steps = (N + 3) // 4
    n_blocks = int(max(1, min(2048, (steps + 15) // 16)))
    partial = torch.empty((n_blocks, P, P), dtype=torch.float64, device=X.device)
    _, s = _ctx(X)
    rc = _raw_call("dx_lr_moments", s, _ptr(X), _ptr(w.to(torch.float64).contiguous()), N, D, _ptr(partial), n_blocks,
                   P)
    if rc != 0:
        raise RuntimeError(f"dx_lr_moments failed rc={rc}")
    return partial.sum(0)[:D, :D]


def lr_encode(X: torch.Tensor, y: torch.Tensor, mean: torch.Tensor, sd: torch.Tensor, wa: float, wb: float):
    """Fused DP encoder on the fp64-MFMA kernel (GPU tensors only): with
    xa_i = [1, (X_i - mean)/sd], returns (sum_i (2y_i-1) xa_i  [D],
    sum_i (wa*y_i + wb) xa_i xa_i^T  [D, D]), D = X.shape[1] + 1."""
    tot = lr_encode_many([X], [y], mean, sd, wa, wb)[0]
    D = X.shape[1] + 1
    return tot[D, :D], tot[:D, :D]


def _lr_blocks(N: int) -> int:
    steps = (N + 3) // 4
    return int(max(1, min(1024, (steps + 15) // 16)))


def _lr_targets(ys: list) -> int:
    """Label columns T of a batch: every entry [N] (or [N, 1]) -> 1, every entry [N, T] -> T."""
    ts = {1 if y.dim() == 1 else int(y.shape[1]) for y in ys if y.dim() in (1, 2)}
    if len(ts) != 1 or any(y.dim() not in (1, 2) for y in ys):
        raise ValueError("lr_encode: the labels of a batch are all [N] or all [N, T] with one T")
    return ts.pop()


# What every DP of an encoder batch shares: raw features dx, D = dx + 1, label
# columns T, slab width P, the device mean / sd and the stream.
_LrPrep = collections.namedtuple("_LrPrep", "dx D T P mean sd stream")


def _lr_prepare(Xs: list, ys: list, mean, sd, wa: float) -> _LrPrep:
    X0 = Xs[0]
    dx = X0.shape[1]
    if dx < 1:
        raise ValueError("lr_encode needs at least one feature")
    T = _lr_targets(ys)
    if T < 1:
        raise ValueError("lr_encode needs at least one label column")
    if T > 1 and float(wa) != 0.0:
        raise ValueError("lr_encode: several label columns share one level 2, so its weight cannot depend on a label")
    mean = torch.as_tensor(mean, dtype=torch.float64).to(X0.device).contiguous()
    sd = torch.as_tensor(sd, dtype=torch.float64).to(X0.device).contiguous()
    assert mean.numel() == dx and sd.numel() == dx
    return _LrPrep(dx, dx + 1, T, _lr_padded(dx + 1 + T), mean, sd, _ctx(X0)[1])


def _lr_labels(p: _LrPrep, X: torch.Tensor, y: torch.Tensor):
    """One DP's labels as the encoder reads them -> (the tensor to keep alive
    until the launch, its pointer, ldy).  T = 1: [N] contiguous.  T > 1: [N, T]
    with unit column stride and a row stride >= T (a column slice of a wider
    matrix is read in place), copied otherwise."""
    assert X.is_cuda and X.dtype == torch.float64 and X.dim() == 2 and X.stride(1) == 1 and X.shape[1] == p.dx
    N = X.shape[0]
    y = y.to(device=X.device, dtype=torch.float64)
    if p.T == 1:
        y = y.reshape(-1).contiguous()
        assert y.numel() == N
        return y, ctypes.c_void_p(y.data_ptr()), 0
    if y.stride(1) != 1 or (N > 1 and y.stride(0) < p.T):
        y = y.contiguous()
    assert y.shape == (N, p.T)
    return y, ctypes.c_void_p(y.data_ptr()), (y.stride(0) if N > 1 else p.T)


def _lr_slab_uninit(D: int, T: int, upper: bool, packed: bool, all_blocks: bool) -> bool:
    """Whether a partial slab may be ``torch.empty`` rather than ``torch.zeros``.

    Invariant: a slab is left uninitialised only when every record block of
    every item is written (``all_blocks``) AND every element the reader will
    read is written; otherwise it is zero-filled, so that what is read but
    unwritten adds nothing.  A shorter DP's trailing blocks in a batch slab
    are never written; every record block of every cell of a window is, with
    zeros where it has no record.  Written are the live tiles: all of [48, 48]
    when P = 48, else row tiles 0..P/16-1 (rows 0..D+T-1: every row tile holds
    a live row) by column tiles 0..ceil(D/16)-1, minus, in the upper plan, the
    tile-blocks strictly below the diagonal of tile-block rows that hold no
    row >= D.  The full reader (``lr_reduce``) reads all of [P, P], of which a
    wide launch leaves the column tiles past D unwritten: with T label columns
    P grows with D + T while the column tiles stay ceil(D/16), so it needs
    P = 48, or the full plan while the two counts agree.  The packed reader
    (``lr_reduce_pack``, ``packed``) reads only (i, j), i <= j < D, which lies
    on or above the diagonal, and rows D..D+T-1 at columns < D, whose
    tile-block rows the upper plan launches whole: all written under either
    plan.  What the upper plan skips and the padding columns are never read
    by it, so they may stay uninitialised.

    Reached today: the batch driver with (upper, packed) = (False, False) and
    (True, True), ``all_blocks`` = the DPs have the same number of record
    blocks; the grouped driver with (False, False), (True, True) and
    (True, False) -- the upper plan under the full reader -- always with
    ``all_blocks``."""
    if not all_blocks:
        return False
    P = _lr_padded(D + T)
    return packed or P == 48 or (not upper and (D + 15) // 16 == P // 16)


def _lr_launch(p: _LrPrep, X: torch.Tensor, labels, wa: float, wb: float, slab: torch.Tensor, n_blocks: int,
               upper: bool, cells=None) -> None:
    """THE native encoder call (dx_lr_encode) into the first ``n_blocks``
    [P, P] blocks of a slab the caller owns: one DP's records X with
    ``labels = _lr_labels(p, X, y)`` in ``n_blocks`` record blocks, or, with
    ``cells = (perm, cell_start, c0, nbc)``, a window of ``n_blocks / nbc`` of
    its cells from cell c0 on.  ``upper``: the packed layout's launch plan,
    which leaves the tile-blocks strictly below the diagonal unwritten."""
    assert slab.is_contiguous() and slab.dtype == torch.float64 and slab.numel() >= n_blocks * p.P * p.P
    perm, cell_start, c0, nbc = cells if cells is not None else (None, None, 0, 0)
    rc = _raw_call("dx_lr_encode", p.stream, ctypes.c_void_p(X.data_ptr()), X.stride(0), X.shape[0], p.dx,
                   _ptr(p.mean), _ptr(p.sd), labels[1], labels[2], p.T, float(wa), float(wb), _ptr(slab), n_blocks,
                   p.P, 1 if upper else 0, _ptr(perm), _ptr(cell_start), c0, nbc)
    if rc != 0:
        raise RuntimeError(f"dx_lr_encode failed rc={rc}")


def _lr_launch_many(Xs: list, ys: list, mean, sd, wa: float, wb: float, upper: bool):
    """One encoder call per DP into one [n, nb, P, P] partial slab (nb = the
    longest DP's record blocks) -> (slab, D).  ``upper``: the packed layout's
    launch plan, for the packed reducer.  Labels [N] (or [N, 1]): level 1 in
    row D.  Labels [N, T], T >= 2 (rows may be strided): level 1 of target t in
    row D + t, level-2 weight the constant ``wb`` (``wa`` must be 0: no
    label-dependent level-2 weight)."""
    p = _lr_prepare(Xs, ys, mean, sd, wa)
    nbs = [_lr_blocks(X.shape[0]) for X in Xs]
    nb = max(nbs)
    alloc = torch.empty if _lr_slab_uninit(p.D, p.T, upper, upper, all(b == nb for b in nbs)) else torch.zeros
    partial = alloc((len(Xs), nb, p.P, p.P), dtype=torch.float64, device=Xs[0].device)
    for i, (X, y) in enumerate(zip(Xs, ys)):
        _lr_launch(p, X, _lr_labels(p, X, y), wa, wb, partial[i], nbs[i], upper)
    return partial, p.D


def _lr_out(what: str, out, shape: tuple, dtype, device) -> torch.Tensor:
    """A reducer's destination: a new tensor, or the caller's after its checks."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(f"{what}: out is {tuple(out.shape)} {out.dtype} on {out.device}"
                         f"{'' if out.is_contiguous() else ', not contiguous'}, needed {shape} {dtype} on {device}")
    return out


def lr_reduce(partial: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Block partials [n, nb, P, P] -> totals [n, P, P] (dx_lr_reduce: block b
    into accumulator b % 4, combined as (s0 + s1) + (s2 + s3)), written into
    ``out`` (contiguous [n, P, P], e.g. a slice of a larger result) if given."""
    assert partial.is_cuda and partial.dtype == torch.float64 and partial.dim() == 4 and partial.is_contiguous()
    n, nb, P, P2 = partial.shape
    assert P == P2 and n >= 1 and nb >= 1
    out = _lr_out("lr_reduce", out, (n, P, P), torch.float64, partial.device)
    _, s = _ctx(partial)
    rc = _raw_call("dx_lr_reduce", s, _ptr(partial), nb, P * P, n, _ptr(out))
    if rc != 0:
        raise RuntimeError(f"dx_lr_reduce failed rc={rc}")
    return out


def lr_encode_many(Xs: list, ys: list, mean, sd, wa: float, wb: float) -> torch.Tensor:
    """``lr_encode`` of several DPs' records with the same standardisation:
    one encoder call per DP into one partial slab, then ONE reduction
    launch (dx_lr_reduce, fixed summation order: a DP's totals are the same
    bits alone or batched) -> [n, P, P] totals with level 2 in [:D, :D] and
    level 1 in row D (D = features + 1; P = 48 up to 46 features, the
    16-padded D + 1 beyond; entries outside those are padding).  Labels
    [N, T], T >= 2: level 1 of target t in row D + t, one shared level 2 with
    the constant weight ``wb``, P = 48 while D + T <= 48 and the 16-padded
    D + T beyond."""
    partial, _ = _lr_launch_many(Xs, ys, mean, sd, wa, wb, False)
    return lr_reduce(partial)


def lr_packed_len(D: int, T: int = 1) -> int:
    """Length of the distinct-coefficient vector: level 1 (D per label column) + the upper triangle of level 2."""
    return T * D + D * (D + 1) // 2


def lr_reduce_pack(partial: torch.Tensor, D: int, precision: float, floats: bool = False, T: int = 1,
                   out: torch.Tensor | None = None, fout: torch.Tensor | None = None):
    """Block partials [n, nb, P, P] (or [nb, P, P]: one item) -> the packed
    int64 vectors [n, D + D(D+1)/2] in ONE launch (dx_lr_reduce_pack): level 1
    from row D, then level 2's upper triangle row-major, summed over the
    blocks in dx_lr_reduce's order, times ``precision``, rounded half away from
    zero.  Reads only (i, j), i <= j < D, and row D of each block.
    ``floats``: also return the unrounded packed fp64 values.  ``T`` label
    columns: [n, T*D + D(D+1)/2], level 1 of target t from row D + t.
    ``out`` / ``fout`` (the latter with ``floats``): contiguous destinations
    of those shapes, e.g. slices of a larger result."""
    if partial.dim() == 3:
        partial = partial[None]
    assert partial.is_cuda and partial.dtype == torch.float64 and partial.dim() == 4 and partial.is_contiguous()
    n, nb, P, P2 = partial.shape
    D, T = int(D), int(T)
    if not (P == P2 and 1 <= D and 1 <= T and D + T <= P and n >= 1 and nb >= 1):
        raise ValueError(f"lr_reduce_pack: slab {tuple(partial.shape)} does not hold rows 0..{D + T - 1}")
    if fout is not None and not floats:
        raise ValueError("lr_reduce_pack: fout without floats")
    shape = (n, lr_packed_len(D, T))
    out = _lr_out("lr_reduce_pack", out, shape, torch.int64, partial.device)
    fout = _lr_out("lr_reduce_pack", fout, shape, torch.float64, partial.device) if floats else None
    _, s = _ctx(partial)
    rc = _raw_call("dx_lr_reduce_pack", s, _ptr(partial), nb, P, D, T, n, float(precision), _ptr(out), _ptr(fout))
    if rc != 0:
        raise RuntimeError(f"dx_lr_reduce_pack failed rc={rc}")
    return (out, fout) if floats else out


def lr_encode_packed_many(Xs: list, ys: list, mean, sd, wa: float, wb: float, precision: float, floats: bool = False):
    """The distinct-coefficient integer vectors of several DPs' records ->
    int64 [n, D + D(D+1)/2] (``floats``: and the unrounded fp64 values): per DP
    the encoder's upper launch plan, then ONE reduce + pack + round launch for
    the batch.  Rows may be strided, any d >= 1, DPs of unequal length.  Entry
    (i, j), i <= j, is the same bits as ``lr_encode_many``'s value there.
    Labels [N, T], T >= 2: int64 [n, T*D + D(D+1)/2], the T level-1 vectors
    (target-major), then the one shared upper triangle."""
    partial, D = _lr_launch_many(Xs, ys, mean, sd, wa, wb, True)
    return lr_reduce_pack(partial, D, precision, floats, _lr_targets(ys))


# Cap of the grouped encoder's partial slab [cells of a window, record blocks
# per cell, P, P]: at P = 48 a block is 18 KB, so the 4096 cells of the largest
# GROUP BY are processed in windows instead of one ~75 MB slab per record block.
LR_CELLS_MAX_SLAB_BYTES = 64 << 20


def _lr_cell_blocks(N: int, G: int) -> int:
    """Record blocks every cell of a DP with N records and G cells gets: those of
    the ungrouped encoder for an even share of the records.  From shapes the
    host knows, never from a cell's size (a cell holding more strides longer);
    one cell: ``_lr_blocks(N)``."""
    return _lr_blocks(-(-int(N) // max(1, int(G))))


def _group_cells(K: torch.Tensor | None, n_rows: int, keys, filters, device, predicate=None):
    """``group_cells`` -> (cells, G)."""
    keys, filters, CK, G, pred = _group_terms("group_cells", K, n_rows, "the records", keys, filters,
                                              predicate=predicate)
    if K is None:
        return torch.zeros(n_rows, dtype=torch.int64, device=device), G
    cell = torch.empty(n_rows, dtype=torch.int64, device=K.device)
    if n_rows == 0:
        return cell, G
    kd = np.ascontiguousarray(np.asarray(keys, dtype=np.int64).reshape(-1))
    fd = np.ascontiguousarray(np.asarray(filters, dtype=np.int64).reshape(-1))
    g, s = _ctx(K)
    rc = _terms_call("dx_group_cells", pred, g, s, _ptr(K, strided=True), K.stride(0) if CK else 0, CK, n_rows,
                     kd.ctypes.data_as(_P), len(keys), fd.ctypes.data_as(_P), len(filters), _ptr(cell))
    if rc == -2:
        raise ValueError("group_cells: the entry refused its arguments")
    if rc != 0:
        raise RuntimeError(f"native op dx_group_cells failed (rc={rc})")
    return cell, G


def group_cells(K: torch.Tensor | None, n_rows: int, keys=(), filters=(), device=None,
                predicate=None) -> torch.Tensor:
    """The cell of every row of the key matrix K [rows, CK] -> [rows] int64
    (dx_group_cells, ``group_moments``' membership rule and argument checks):
    the mixed-radix group index over ``keys``, or G (the number of groups) for a
    row that a filter term (with ``predicate``: the formula over the filters'
    atoms) or an out-of-range key digit drops.  K is read in place through its
    row stride; None without keys and filters (one cell)."""
    return _group_cells(K, n_rows, keys, filters, device, predicate)[0]


def lr_cell_plan(K: torch.Tensor | None, n_rows: int, keys=(), filters=(), device=None, predicate=None):
    """The cell plan of one DP's records -> (perm, cell_start, G): the rows that
    belong to a cell, grouped by cell with the record order kept inside a cell
    (a stable sort of ``group_cells``; dropped rows sort behind the last cell),
    and the cells' bounds in it, [G + 1].  Device ops only: nothing is copied
    to the host."""
    cell, G = _group_cells(K, n_rows, keys, filters, device, predicate)
    ids, perm = torch.sort(cell, stable=True)
    cell_start = torch.searchsorted(ids, torch.arange(G + 1, dtype=torch.int64, device=cell.device))
    return perm, cell_start, G


def _lr_cells_run(Xs: list, ys: list, Ks: list, mean, sd, wb: float, keys, filters, upper: bool, max_slab_bytes,
                  pack=None, predicate=None):
    """The grouped encoder DP by DP and window by window -> (out, fout).  Every
    window's [cw, nbc, P, P] slab is reduced straight into ``out[dp, c0:c0 +
    cw]``: by ``lr_reduce`` into totals [n, G, P, P], or, with ``pack =
    (precision, floats)``, by ``lr_reduce_pack`` into the packed int64 vectors
    [n, G, T*D + D(D+1)/2] (and their unrounded values ``fout``).  A DP
    without records is zeros."""
    p = _lr_prepare(Xs, ys, mean, sd, 0.0)
    if len(Ks) != len(Xs) or len(ys) != len(Xs):
        raise ValueError("lr_encode_cells: one label tensor and one key matrix (or None) per DP")
    dev = Xs[0].device
    precision, floats = pack if pack is not None else (None, False)
    alloc = torch.empty if _lr_slab_uninit(p.D, p.T, upper, pack is not None, True) else torch.zeros
    out = fout = None
    for i, (X, y, K) in enumerate(zip(Xs, ys, Ks)):
        labels = _lr_labels(p, X, y)
        N = X.shape[0]
        if K is not None and K.device != dev:
            raise ValueError(f"native op mixes devices {dev} and {K.device}")
        perm, cell_start, G = lr_cell_plan(K, N, keys, filters, dev, predicate)
        if out is None:  # G is the first plan's: the keys' cardinalities, the same for every DP
            if pack is None:
                out = torch.empty((len(Xs), G, p.P, p.P), dtype=torch.float64, device=dev)
            else:
                out = torch.empty((len(Xs), G, lr_packed_len(p.D, p.T)), dtype=torch.int64, device=dev)
                fout = torch.empty(out.shape, dtype=torch.float64, device=dev) if floats else None
        if N == 0:
            out[i].zero_()
            if fout is not None:
                fout[i].zero_()
            continue
        nbc = _lr_cell_blocks(N, G)
        cw = int(max(1, min(G, int(max_slab_bytes) // (nbc * p.P * p.P * 8))))
        slab = alloc((cw, nbc, p.P, p.P), dtype=torch.float64, device=dev)
        for c0 in range(0, G, cw):
            w = min(cw, G - c0)
            _lr_launch(p, X, labels, 0.0, wb, slab, w * nbc, upper, (perm, cell_start, c0, nbc))
            if pack is None:
                lr_reduce(slab[:w], out=out[i, c0:c0 + w])
            else:
                lr_reduce_pack(slab[:w], p.D, precision, floats, p.T, out=out[i, c0:c0 + w],
                               fout=fout[i, c0:c0 + w] if floats else None)
    return out, fout


def lr_encode_cells_many(Xs: list, ys: list, Ks: list, mean, sd, wb: float, keys=(), filters=(), *,
                         upper: bool = False, max_slab_bytes: int = LR_CELLS_MAX_SLAB_BYTES,
                         predicate=None) -> torch.Tensor:
    """``lr_encode_many`` per cell of a WHERE / GROUP BY over the DPs' records
    (the fused fp64-MFMA encoder with the rows read through a cell plan) ->
    [n, G, P, P] totals: for cell c of DP i level 2 (weight
    ``wb``) in [:D, :D] and level 1 in rows D..D+T-1, summed over the records of
    the cell; an empty cell is zeros.  ``Ks[i]`` [N_i, CK] int64 holds the key
    and filter columns of DP i's records row for row (read in place through its
    row stride; None without keys and filters); ``keys`` / ``filters`` /
    ``predicate`` and their limits are ``group_moments``'.  Per DP the cells are encoded in windows whose
    partial slab stays within ``max_slab_bytes``; every window is finished by
    dx_lr_reduce with the cells as items, so a cell is the same bits whatever
    the windows and whichever DPs share the batch.  ``upper``: the packed
    layout's launch plan (what it skips is left zero or unwritten).  One cell
    and no filter: ``lr_encode_many``'s bits."""
    return _lr_cells_run(Xs, ys, Ks, mean, sd, wb, keys, filters, upper, max_slab_bytes, predicate=predicate)[0]


def lr_encode_cells_packed_many(Xs: list, ys: list, Ks: list, mean, sd, wb: float, keys=(), filters=(),
                                precision: float = 1.0, *, floats: bool = False,
                                max_slab_bytes: int = LR_CELLS_MAX_SLAB_BYTES, predicate=None):
    """``lr_encode_packed_many`` per cell: the distinct-coefficient integer
    vectors -> int64 [n, G, T*D + D(D+1)/2] (``floats``: and the unrounded fp64
    values), the encoder's upper launch plan per window and ONE reduce + pack +
    round launch (dx_lr_reduce_pack) per window with the cells as items.  Entry
    (i, j), i <= j, of a cell is the same bits as ``lr_encode_cells_many``'s."""
    out, fout = _lr_cells_run(Xs, ys, Ks, mean, sd, wb, keys, filters, True, max_slab_bytes, (precision, floats),
                              predicate)
    return (out, fout) if floats else out


# ----------------------------------------------------------------------------- range proofs (K15/K16)
def rp_prove_a(negsB_aff, V_aff, t_sc, gt_table, S: int, L: int) -> torch.Tensor:
    n = _rows(V_aff, 32)
    out = torch.empty((n, 96), dtype=torch.int32, device=V_aff.device)
    g, s = _ctx(negsB_aff, V_aff, t_sc, gt_table)
    _call("dx_rp_prove_a", g, s, _ptr(negsB_aff), _ptr(V_aff), _ptr(t_sc), _ptr(gt_table), _ptr(out), n, S, L)
    return out


def rp_prove_a_tab(gphi_tables, tab_idx, e_sc, t_sc, gt_table, S: int, L: int, wbits: int = 8) -> torch.Tensor:
    """wbits = 8: gphi_tables in the 8-bit comb layout; 4: the 4-bit layout
    (gt_fb4_table); 7: the GLS-2 signed 8-bit layout (gt_gls8_table)."""
    assert wbits in (4, 7, 8)
    n = _rows(e_sc, 8)
    out = torch.empty((n, 96), dtype=torch.int32, device=e_sc.device)
    g, s = _ctx(gphi_tables, tab_idx, e_sc, t_sc, gt_table)
    if wbits == 7:
        assert tab_idx.dtype == torch.int32 and tab_idx.numel() == n and n % (S * L) == 0
        t16 = gt16_table(e_sc.device) if e_sc.is_cuda else None                # gT^t in 17 steps
        tmp = torch.empty_like(out) if g else None                             # the finish pass's prefixes and norms
        _call("dx_rp_prove_a_gls8", g, s, _ptr(gphi_tables), _ptr(tab_idx), _ptr(e_sc), _ptr(t_sc),
              _ptr(t16 if t16 is not None else gt_table), _ptr(out), n, S, L, int(t16 is not None), _ptr(tmp))
        return out
    _call("dx_rp_prove_a_tab", g, s, _ptr(gphi_tables), _ptr(tab_idx), _ptr(e_sc), _ptr(t_sc), _ptr(gt_table),
          _ptr(out), n, S, L, wbits)
    return out


def rp_challenges(C_aff: torch.Tensor, b_words: torch.Tensor, y_words: torch.Tensor,
                  cols: torch.Tensor) -> torch.Tensor:
    """Range-proof challenges SHA3-512(B || C_p || Y_col) mod r -> [n, 8]
    canonical scalars (dx_keccak.hip).  b_words [16] and y_words [n_cols, 16]
    are the 64-byte point encodings viewed as little-endian int32 words."""
    n = _rows(C_aff, 16)
    assert cols.dtype == torch.int32 and cols.numel() == n and b_words.numel() == 16
    out = torch.empty((n, 8), dtype=torch.int32, device=C_aff.device)
    g, s = _ctx(C_aff, b_words, y_words, cols)
    _call("dx_rp_challenges", g, s, _ptr(C_aff), _ptr(b_words), _ptr(y_words), _ptr(cols), _ptr(out), n)
    return out


# GLV batch weights (csrc/kernels/dx_glv.hip): rho = a + b * GLV_LAMBDA mod r with
# a, b 32-bit; phi(x, y) = (GLV_BETA x, y) = [GLV_LAMBDA] on G1; x^GLV_LAMBDA =
# x^(p^8) on GT.  Both constants are checked against the oracle in the tests.
GLV_BETA = 0x59E26BCEA0D48BACD4F263F1ACDB5C4F5763473177FFFFFE
GLV_LAMBDA = 0xB3C4D79D41A917585BFC41088D8DAAA78B17EA66B99C90DD
_glv_consts: dict = {}


def _glv_const(kind: str, device) -> torch.Tensor:
    from ..crypto import bn254 as _bn

    key = (kind, str(device))
    if key not in _glv_consts:
        if kind == "beta":
            v = _bn.to_tensor(_bn.ints_to_limbs([_bn.mont(GLV_BETA)]), device)
        else:
            v = _bn.to_tensor(_bn.ints_to_limbs([GLV_LAMBDA]), device)
        _glv_consts[key] = _bn.publish(v.contiguous())
    return _glv_consts[key]


def prg_glv(key: bytes, n: int, device):
    """``glv_weights(n, device, raw=prg_scalars(key, n, device))`` in ONE
    launch (csrc/kernels/dx_hash.hip dx_prg_glv) -> (ab [n, 2], rho [n, 8])."""
    device = torch.device(device)
    ab = torch.empty((max(0, n), 2), dtype=torch.int32, device=device)
    rho = torch.empty((max(0, n), 8), dtype=torch.int32, device=device)
    if n <= 0:
        return ab, rho
    k = np.frombuffer(key[:32], dtype="<u4").copy()
    lam = np.asarray(_lambda_limbs(), dtype=np.uint32)
    g, s = _ctx(ab)
    _call("dx_prg_glv", g, s, k.ctypes.data_as(ctypes.c_void_p), 0, lam.ctypes.data_as(ctypes.c_void_p), _ptr(ab),
          _ptr(rho), n)
    return ab, rho


def prg_bits(key: bytes, n: int, bits: int, device) -> torch.Tensor:
    """``coins.mask_bits(prg_scalars(key, n, device), bits)`` in ONE launch."""
    device = torch.device(device)
    out = torch.empty((max(0, n), 8), dtype=torch.int32, device=device)
    if n <= 0:
        return out
    k = np.frombuffer(key[:32], dtype="<u4").copy()
    g, s = _ctx(out)
    _call("dx_prg_bits", g, s, k.ctypes.data_as(ctypes.c_void_p), 0, int(bits), _ptr(out), n)
    return out


def _lambda_limbs() -> list:
    from ..crypto import bn254 as _bn

    return [int(x) for x in _bn.ints_to_limbs([GLV_LAMBDA]).reshape(-1)]


def glv_weights(n: int, device, raw: torch.Tensor | None = None):
    """n GLV batch weights: (ab [n, 2] int32 = the 32-bit halves (a, b),
    rho [n, 8] = a + b * GLV_LAMBDA as canonical scalars); ``raw``: [n, 8]
    uniform scalars to take the halves from (a verifier's own coins)."""
    from ..crypto import bn254 as _bn

    if raw is None:
        raw = _bn.random_scalars(n, device)
    ab = raw[:, :2].contiguous()
    a = torch.zeros_like(raw)
    b = torch.zeros_like(raw)
    a[:, 0] = ab[:, 0]
    b[:, 0] = ab[:, 1]
    rho = fr_arith(FR_ADD, a, fr_arith(FR_MUL, b, _glv_const("lambda", device)))
    return ab, rho


def g1_mul_glv(pts_jac: torch.Tensor, ab: torch.Tensor) -> torch.Tensor:
    """(a_i + b_i GLV_LAMBDA) P_i for 32-bit halves ab [n, 2] (``glv_weights``)
    -> Jacobian [n, 24]: 32 doublings of a joint 2-bit-window ladder over
    (P, phi(P)) instead of 64 (csrc/kernels/dx_glv.hip).  GPU; on the host
    the full scalars go through ``g1_mul``."""
    n = _rows(ab, 2)
    np_ = _rows(pts_jac, 24)
    assert np_ in (1, n)
    if not ab.is_cuda:
        a = torch.zeros((n, 8), dtype=torch.int32)
        b = torch.zeros((n, 8), dtype=torch.int32)
        a[:, 0], b[:, 0] = ab[:, 0], ab[:, 1]
        rho = fr_arith(FR_ADD, a, fr_arith(FR_MUL, b, _glv_const("lambda", "cpu")))
        return g1_mul(pts_jac, rho)
    out = torch.empty((n, 24), dtype=torch.int32, device=ab.device)
    _, s = _ctx(pts_jac, ab)
    rc = _raw_call("dx_g1_mul_glv", s, _ptr(pts_jac.contiguous()), _ptr(ab.contiguous()),
                   _ptr(_glv_const("beta", ab.device)), _ptr(out), n, int(np_ == 1 and n > 1))
    if rc:
        raise RuntimeError(f"dx_g1_mul_glv failed rc={rc}")
    return out


def g1_aff_to_uv_(aff: torch.Tensor) -> torch.Tensor:
    """In place: affine (x, y) rows -> (x/y, 1/y) (infinity stays zeros)."""
    g, s = _ctx(aff)
    _call("dx_g1_aff_to_uv", g, s, _ptr(aff), _rows(aff, 16))
    return aff


FOLD_P_ALIGN = 8  # verifier blocks are padded to 64 K * 8 items (XCD-paired block mapping)


def rp_fold_ncoeffs(V_aff: torch.Tensor) -> torch.Tensor:
    """Normalised line image of every V's Miller loop (no P): per V and step
    (c1/c0, c3/c0) -> flat int32 [steps * 8 * m * 4] (csrc/kernels/dx_fold.hip).
    GPU only."""
    m = _rows(V_aff, 32)
    assert V_aff.is_cuda and V_aff.is_contiguous()
    steps = _load().dx_fold_steps()
    img = torch.empty((steps * 8 * m * 4,), dtype=torch.int32, device=V_aff.device)
    scratch = torch.empty((2 * steps * 4 * m * 4,), dtype=torch.int32, device=V_aff.device)
    _, s = _ctx(V_aff)
    _call("dx_rp_ncoeffs", s, _ptr(V_aff), _ptr(img), _ptr(scratch), m)
    return img


def rp_fold_accum_n(img: torch.Tensor, UV: torch.Tensor, V_aff: torch.Tensor, period: int, G: int,
                    K: int = 4) -> torch.Tensor:
    """One-lane normalised accumulation: G verifiers' (u, v) point images
    (UV[v * period + q], q < m) against one normalised line image, K items
    per lane sharing one accumulator -> [G * period / (64 K), 96] partial
    products, verifier-major."""
    m = _rows(V_aff, 32)
    assert _rows(UV, 16) == G * period and period >= m and period % (64 * K * FOLD_P_ALIGN) == 0
    assert img.numel() == _load().dx_fold_steps() * 8 * m * 4
    fb = torch.empty((G * period // (64 * K), 96), dtype=torch.int32, device=UV.device)
    _, s = _ctx(img, UV, V_aff)
    _call("dx_rp_accum_n", s, _ptr(img), _ptr(UV), _ptr(V_aff), _ptr(fb), m, period, G, K)
    return fb


def rp_fold_accum_coop_raw(coef: torch.Tensor, P_aff: torch.Tensor, V_aff: torch.Tensor, period: int,
                           G: int) -> torch.Tensor:
    """Three-lane accumulation over the RAW line coefficients (``rp_fold_coeffs``,
    no normalising pass) and affine points P -> [G * period / 64, 96].  GPU only."""
    m = _rows(V_aff, 32)
    n = G * period
    assert _rows(P_aff, 16) == n and period >= m and period % 64 == 0
    assert coef.numel() == _load().dx_fold_steps() * 12 * m * 4  # one step count (pairing.h) sizes both folds' images
    f = torch.empty((n, 96), dtype=torch.int32, device=P_aff.device)
    _, s = _ctx(coef, P_aff, V_aff)
    _call("dx_ufold_coop_raw", s, _ptr(coef), _ptr(P_aff), _ptr(V_aff), _ptr(f), m, period, n)
    x = f.view(64, n // 64, 96)  # written lane-major by the kernel: item t at row (t % 64, t // 64)
    while x.shape[0] > 1:
        x = _gt_prod_level(x, 8)
    return x.view(n // 64, 96)


def gt_frob8(a: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """a^(p^8) per row (= a^GLV_LAMBDA on GT); ``out``: a contiguous
    destination of a's shape (e.g. the second half of a stacked image)."""
    out = torch.empty_like(a) if out is None else out
    assert out.is_contiguous() and out.shape == a.shape
    g, s = _ctx(a)
    _call("dx_gt_frob8", g, s, _ptr(a.contiguous()), _ptr(out), _rows(a, 96))
    return out


def gt_beta_rows(a: torch.Tensor, rows_per_inv: int | None = None) -> torch.Tensor:
    """Unitary GT elements a [m, 96] -> beta2 [2m, 48]: row i the torus image
    (1 + g) / h of a_i = g + h w (the limbs ``gt_t2_compress`` writes), row
    m + i the image of frob^8(a_i); a row with h = 0 (a_i = 1) is all zero in
    both halves, the skip mark of ``gt_beta_slice_prod``
    (csrc/kernels/dx_me_torus.hip).  ``rows_per_inv`` rows share one Fp6
    inversion (default: up to 8, no more than keeps two waves per SIMD)."""
    m = _rows(a, 96)
    if rows_per_inv is None:
        rows_per_inv = 8 if a.device.type != "cuda" else max(1, min(8, m // (1024 * 64 * 2)))
    out = torch.empty((2 * m, 48), dtype=torch.int32, device=a.device)
    g, s = _ctx(a)
    _call("dx_gt_beta_rows", g, s, _ptr(a.contiguous()), _ptr(out), m, int(rows_per_inv))
    return out


def gt_pi(y: torch.Tensor) -> torch.Tensor:
    """Numerators y [n, 96] (non-zero Fp12 values) -> pi(y) = y / conj(y), the
    canonical unitary values (csrc/bn254/gt_torus.h)."""
    out = torch.empty_like(y)
    g, s = _ctx(y)
    _call("dx_gt_pi", g, s, _ptr(y.contiguous()), _ptr(out), _rows(y, 96))
    return out


def rp_fold_coeffs(V_aff: torch.Tensor) -> torch.Tensor:
    """The raw line coefficients (c0, c1, c3) of every V's Miller loop (no P)
    -> flat int32 image [steps * 12 * m * 4]; several verifiers folding the
    same proofs share it (``rp_fold_accum_coop_raw`` evaluates at their P).
    GPU only."""
    m = _rows(V_aff, 32)
    assert V_aff.is_cuda and V_aff.is_contiguous()
    coef = torch.empty((_load().dx_fold_steps() * 12 * m * 4,), dtype=torch.int32, device=V_aff.device)
    _, s = _ctx(V_aff)
    _call("dx_rp_coeffs", s, _ptr(V_aff), _ptr(coef), m)
    return coef


# ----------------------------------------------------------------------------- U side (verifier mode "msm")
# csrc/kernels/dx_rpmsm.hip: range-proof batch verification by bilinearity
# (the bucket plans of its three multi-scalar products: msm.py)
G2_JOINT_ENTRIES = 15


def g2_joint_table(V_aff: torch.Tensor, sign: torch.Tensor | None = None) -> torch.Tensor:
    """Per V: the 15 affine points da V + db [lambda] V ((da, db) in [0, 3]^2,
    not both 0) -> [m * 15, 32]; the U-combination kernel's window table.
    ``sign`` (int32 [m]): where nonzero the second axis is -[lambda] V (the
    table of a GLV-split scalar k1 - |k2| lambda)."""
    m = _rows(V_aff, 32)
    out = torch.empty((m * G2_JOINT_ENTRIES, 32), dtype=torch.int32, device=V_aff.device)
    if sign is None:
        g, s = _ctx(V_aff)
        _call("dx_g2_joint_table", g, s, _ptr(V_aff.contiguous()), _ptr(out), m)
        return out
    assert sign.dtype == torch.int32 and sign.numel() == m
    g, s = _ctx(V_aff, sign)
    _call("dx_g2_joint_table_signed", g, s, _ptr(V_aff.contiguous()), _ptr(sign.contiguous()), _ptr(out), m)
    return out


def rp_u_joint(table: torch.Tensor, ab: torch.Tensor, n_groups: int, G: int, L: int, out: torch.Tensor,
               pad: int, pos: torch.Tensor | None = None) -> torch.Tensor:
    """out[v*pad + q] = affine(sum_j (a + b lambda)_{v, q*L+j} V_{q*L+j}) for every
    verifier v < G and group q < n_groups (ab [G * n_groups * L, 2] int32);
    ``pos`` (int64 [G * n_groups], rows of ``out``): the row of (v, q) instead."""
    assert _rows(table, 32) == n_groups * L * G2_JOINT_ENTRIES and _rows(ab, 2) == G * n_groups * L
    assert out.is_contiguous() and pad >= n_groups
    if pos is None:
        assert _rows(out, 32) >= (G - 1) * pad + n_groups
    else:
        assert pos.dtype == torch.int64 and pos.numel() == G * n_groups and pos.device == out.device
    g, s = _ctx(table, ab, out)
    # a small batch (a pool helper's 1/W slice) splits each combination over
    # 2 or 4 threads so the launch still fills the chip (~2 waves per SIMD)
    n = G * n_groups
    sp = 1 if (not g or n >= 131072) else (2 if n >= 65536 else 4)
    sp = min(sp, L)
    if sp > 1:
        tmp = torch.empty((n * sp, 48), dtype=torch.int32, device=out.device)
        _call("dx_rp_u_joint_split", g, s, _ptr(table), _ptr(ab.contiguous()), _ptr(out), n_groups, G, L, pad, sp,
              _ptr(tmp), _ptr(pos))
        return out
    _call("dx_rp_u_joint", g, s, _ptr(table), _ptr(ab.contiguous()), _ptr(out), n_groups, G, L, pad, _ptr(pos))
    return out


def rp_u_group_lanes(n: int, on_gpu: bool) -> int:
    """Lanes per key-group combination: the (VN, group) pairs of a query are
    far fewer than the chip's lanes, and a group's chain (126 doublings + ~60
    additions per member) is long -- split until the launch has ~32k lanes.
    The rule rests on the kernel's stand-alone time only.  At the 1-GPU
    query (18,630 pairs of 10 members), alone on the chip: 1 lane 19.3 ms,
    2 lanes 10.7 ms, 4 lanes 11.0 ms.  End to end, beside the other streams'
    kernels, 1 and 2 lanes are indistinguishable; 2 is kept for a U stream
    that runs alone.  Each split repeats the group's doublings, and 4 lanes
    cost 3 to 5 ms more per query (tools/ygroup_micro.py,
    profiles/ygroup/README.md)."""
    if not on_gpu:
        return 1
    sp = 1
    while sp < 16 and n * sp < 32768:
        sp *= 2
    return sp


def rp_u_group(table: torch.Tensor, split: torch.Tensor, idx: torch.Tensor, start: torch.Tensor,
               length: torch.Tensor, G: int, nq: int, S: int, out: torch.Tensor, pad: int,
               pos: torch.Tensor | None = None, sp: int | None = None) -> torch.Tensor:
    """Key-group combinations: out[v*pad + g] = affine(sum_k c_(q_k // S) U_(v, q_k)),
    q_k = idx[start[g] + k], k < length[g], for every verifier v < G and
    group g.  ``table``: the signed joint table of the G * nq rows U (sign of
    row v nq + q: ``split[q // S, 8]``); ``split`` [n, 9]: ``glv_split`` of the
    proofs' challenges c; ``idx`` (int32, values < nq) lists the groups'
    members.  ``pos`` as in ``rp_u_joint``; ``sp``: lanes per (v, g)
    (a power of two <= 64; chosen by ``rp_u_group_lanes`` when None)."""
    ng = start.numel()
    assert _rows(table, 32) == G * nq * G2_JOINT_ENTRIES and _rows(split, 9) * S >= nq
    assert idx.dtype == torch.int32 and start.dtype == torch.int64 and length.dtype == torch.int32
    assert length.numel() == ng and out.is_contiguous() and pad >= ng
    if pos is None:
        assert _rows(out, 32) >= (G - 1) * pad + ng
    else:
        assert pos.dtype == torch.int64 and pos.numel() == G * ng and pos.device == out.device
    g, s = _ctx(table, split, idx, start, length, out)
    if sp is None:
        sp = rp_u_group_lanes(G * ng, bool(g))
    assert sp >= 1 and 64 % sp == 0
    tmp = None if g else torch.empty((G * ng * sp, 48), dtype=torch.int32)
    _call("dx_rp_u_group", g, s, _ptr(table), _ptr(split.contiguous()), _ptr(idx), _ptr(start), _ptr(length),
          _ptr(out), ng, G, nq, S, sp, pad, _ptr(pos), _ptr(tmp))
    return out


_gt_one_cache: dict = {}


def gt_one(device) -> torch.Tensor:
    """Fp12 one (Montgomery limbs: c0.c0.c0 = R mod p)."""
    key = str(device)
    if key not in _gt_one_cache:
        from ..crypto import bn254 as _bn

        t = np.zeros((1, 96), dtype=np.uint32)
        t[0, :8] = _bn.ints_to_limbs([_bn.mont(1)])[0]
        _gt_one_cache[key] = _bn.publish(_bn.to_tensor(t, device))
    return _gt_one_cache[key]


def _pow2_scalar(c: int) -> torch.Tensor:
    t = torch.zeros((1, 8), dtype=torch.int32)
    t[0, c // 32] = 1 << (c % 32)
    return t


def _finish_prod_on_host(parts: torch.Tensor) -> torch.Tensor:
    """Product of [n, 96] GT partials: 8-way GPU levels while n > 256, then the
    rest on the host pool (a lone GPU lane runs an Fp12 chain latency-bound,
    ~30x slower than one host core).  Returns a [1, 96] HOST tensor."""
    cur = parts.view(-1, 1, 96)
    while cur.shape[0] > 256:
        cur = _gt_prod_level(cur, 8)
    return gt_prod(cur.cpu(), chunk=4).view(1, 96)


def _gt_prod_level(x: torch.Tensor, ch: int) -> torch.Tensor:
    n_items, n_groups = x.shape[0], x.shape[1]
    n_chunks = (n_items + ch - 1) // ch
    out = torch.empty((n_chunks, n_groups, 96), dtype=torch.int32, device=x.device)
    g, s = _ctx(x)
    _call("dx_gt_prod_chunks", g, s, _ptr(x.contiguous()), _ptr(out), n_items, n_groups, ch)
    return out


# the verifier's multi-scalar products (bucket plans over the ops above): last, msm.py imports from this module
from .msm import (G2_CHUNK, capture_keep, check_overflow, g1_msm, g1_msm_device, g1_msm_finish,  # noqa: E402,F401
                  g1_msm_grouped, g1_msm_launch, g1_msm_plan, g1_slice_sum, g2_chunk_weight, g2_msm_device,
                  g2_msm_finish, g2_msm_launch, g2_msm_run, g2_slice_sum, gt_beta_slice_prod, gt_chunk_weight,
                  gt_slice_prod, me_window, multi_exp_device, multi_exp_grouped, multi_exp_grouped_finish,
                  multi_exp_plan, rp_msm_uv)
