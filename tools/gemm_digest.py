"""sha256 of the outputs of the MFMA GEMM kernels (gemm.hip: the 64 x 64 kernel, the tile
kernel, the fused-Adam epilogue and the Conv1D input gradient) on the shapes their tests use.

One line `case sha256` per output array, over the array's bytes. Two builds of the library
whose kernels issue the same f32 operations in the same order print the same listing:

    XA_LIB=<the other build's libxagents_hip.so> python tools/gemm_digest.py > a.txt
    python tools/gemm_digest.py > b.txt
    diff a.txt b.txt

Only the public surface (layers.gemm / gemm_adam, xa_conv1d_dgrad through _lib.call) is
used, so the same file runs against older builds. The tile-kernel cases and their operands
are the ones of tests/test_gpu_layers.py::test_gemm_tile_kernel_operand_forms.
"""
import hashlib
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

from xagents_amd import _lib  # noqa: E402
from xagents_amd.layers import adam_apply, fold_bias_ok, gemm, gemm_adam  # noqa: E402
import test_gpu_layers as T  # noqa: E402

DEV = torch.device('cuda:0')

# test_gemm_plain_bias_relu_split with K <= 5000 (both force_small values)
PLAIN = [c for c in T._SHAPES if c[2] <= 5000]
TRANSPOSES = [(70, 45, 33), (260, 300, 77), (700, 60, 45), (60, 400, 50)]
ONES_ROW = [(512, 6, 64, False), (129, 70, 3001, False), (5, 7, 9, True)]
ADAM = [(128, 68, 33), (129, 68, 33), (3000, 512, 40), (64, 8, 100)]
DGRAD = [(7, 20, 32, 64, 4, 2), (5, 9, 64, 64, 3, 1), (3, 24, 96, 8, 5, 2), (4, 11, 17, 12, 2, 3),
         (130, 84, 32, 64, 8, 4)]


def emit(case, t):
    torch.cuda.synchronize()
    digest = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes())
    print(f'{case} {digest.hexdigest()}', flush=True)


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in arrays]


def tile():
    for shape, M, N, K, splits, af, bf, gb in T._TILE_CASES:
        C, _ = T._tile_gemm(DEV, M, N, K, splits, af, bf, gb)
        emit(f'tile{shape}_{M}x{N}x{K}_s{splits}_{af}_{bf}_gb{int(gb)}', C)


def plain():
    for M, N, K, splits in PLAIN:
        rng = np.random.default_rng(M + N + K)
        ta, tb, tbias = dev(rng.normal(size=(M, K)).astype(np.float32),
                            rng.normal(size=(K, N)).astype(np.float32),
                            rng.normal(size=N).astype(np.float32))
        ws = torch.empty(splits * M * N + 1, device=DEV)
        for small in (False, True):
            C = torch.empty(M, N, device=DEV)
            gemm(M, N, K, ta.data_ptr(), tb.data_ptr(), C.data_ptr(), a_m=(1, K, 0), b_ks=N,
                 b_ns=1, ldc=N, bias=tbias.data_ptr(), act=_lib.XA_ACT_RELU, workspace=ws,
                 splits=splits, force_small=small)
            emit(f'plain_{M}x{N}x{K}_s{splits}_small{int(small)}', C)


def transposes():
    for M, N, K in TRANSPOSES:
        rng = np.random.default_rng(3)
        ta, tb, tg, C = dev(rng.normal(size=(K, M)).astype(np.float32),
                            rng.normal(size=(N, K)).astype(np.float32),
                            rng.normal(size=(M, N)).astype(np.float32),
                            rng.normal(size=(M, N)).astype(np.float32))
        gemm(M, N, K, ta.data_ptr(), tb.data_ptr(), C.data_ptr(), a_m=(1, 1, 0), a_k=(1, M, 0),
             b_ks=1, b_ns=K, ldc=N, gate=tg.data_ptr(), ld_gate=N, beta=True, splits=1)
        emit(f'transposed_{M}x{N}x{K}', C)
        rows, W, Cc, k, s = 11 + M // 10, 20, 3, 4, 2
        P = (W - k) // s + 1
        tx, tw = dev(rng.integers(0, 256, size=(rows, W, Cc), dtype=np.uint8),
                     rng.normal(size=(k * Cc, 8)).astype(np.float32))
        out = torch.empty(rows * P, 8, device=DEV)
        gemm(rows * P, 8, k * Cc, tx.data_ptr(), tw.data_ptr(), out.data_ptr(), a_u8=True,
             a_m=(P, W * Cc, s * Cc), b_ks=8, b_ns=1, ldc=8, splits=1)
        emit(f'u8_im2col_{rows * P}x8x{k * Cc}', out)


def ones_row():
    for M, N, K, beta in ONES_ROW:
        rng = np.random.default_rng(M + N + K)
        tx, tdz, C = dev(rng.normal(size=(K, M)).astype(np.float32),
                         rng.normal(size=(K, N)).astype(np.float32),
                         rng.normal(size=(M + 1, N)).astype(np.float32))
        s = _lib.load().xa_gemm_splits(M + 1, N, K)
        ws = torch.empty(max(s, 1) * (M + 1) * N + 1, device=DEV)
        gemm(M + 1, N, K, tx.data_ptr(), tdz.data_ptr(), C.data_ptr(), a_m=(1, 1, 0),
             a_k=(1, M, 0), b_ks=N, b_ns=1, ldc=N, beta=beta, workspace=ws, a_ones_row=True)
        emit(f'ones_row_{M}x{N}x{K}_beta{int(beta)}', C)


def adam():
    class Opt:
        learning_rate, beta_1, beta_2, epsilon = 1e-3, 0.9, 0.999, 1e-7

    for M, N, K in ADAM:
        if not fold_bias_ok(M, N, K):
            print(f'adam_{M}x{N}x{K} not on the 64 x 64 kernel', flush=True)
            continue
        rng = np.random.default_rng(M + N + K)
        X, dZ, th = dev(rng.normal(size=(K, M)).astype(np.float32),
                        rng.normal(size=(K, N)).astype(np.float32),
                        rng.normal(size=(M + 1) * N).astype(np.float32))
        m, v, g = torch.zeros_like(th), torch.zeros_like(th), torch.empty_like(th)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        for _ in range(2):
            _lib.call('xa_adam_step_bump', step.data_ptr(), _lib.stream())
            gemm_adam(M + 1, N, K, X.data_ptr(), dZ.data_ptr(), g.data_ptr(),
                      adam_apply(th, m, v, step, Opt, 0), a_m=(1, 1, 0), a_k=(1, M, 0), b_ks=N,
                      b_ns=1, ldc=N, a_ones_row=True)
        for name, t in (('theta', th), ('m', m), ('v', v), ('g', g)):
            emit(f'adam_{M}x{N}x{K}_{name}', t)


def dgrad():
    for rows, W, C, F, k, s in DGRAD:
        rng = np.random.default_rng(rows * W + C)
        P = (W - k) // s + 1
        tdy, tw, tg = dev(rng.normal(size=(rows, P, F)).astype(np.float32),
                          rng.normal(size=(k, C, F)).astype(np.float32),
                          rng.normal(size=(rows, W, C)).astype(np.float32))
        for tag, g_ptr in (('plain', None), ('gated', tg.data_ptr())):
            out = torch.full((rows, W, C), float('nan'), device=DEV)
            _lib.call('xa_conv1d_dgrad', tdy.data_ptr(), tw.data_ptr(), rows, P, k, s, C, F, W,
                      g_ptr, out.data_ptr(), _lib.stream())
            emit(f'dgrad_{rows}x{W}x{C}_F{F}_k{k}_s{s}_{tag}', out)


def main():
    if os.environ.get('XA_LIB'):  # another build of the library instead of the product
        _lib._lib = _lib.load(os.environ['XA_LIB'])
    for group in (tile, plain, transposes, ones_row, adam, dgrad):
        group()


if __name__ == '__main__':
    main()
