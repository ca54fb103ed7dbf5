"""Numpy float64 model of THE reduction order of the record kernels (isdf_amd/csrc/block_reduce.h, reduce.hip) -- TEST
INFRASTRUCTURE.  Every function takes the terms along axis 0 and any number of columns behind it; each column is reduced on its
own, in the order the header promises (include/isdf_hip.h: "bit-identical from run to run", "the blocks in block order"):

    block_sum            the 256 threads of a block: lanes by shuffle halving, then the four waves in wave order
    grid_stride_record   per-block partial records of a grid-stride kernel (sdf_metrics, region_metrics, pose_system; with no cap
                         on the blocks: nn_finish, tri_finish)
    close_strided        reduce_partials_kernel: thread k takes partials k, k + 256, .. ascending, then the block's order
    close_serial         pose_close_kernel: one thread adds a pose's partials in block order
"""
import numpy as np


def block_sum(x256):
    """[256, ...] -> [...]: wave_reduce (offsets 32, 16, .., 1 by __shfl_down) and waves_combine ((w0 + w1) + w2) + w3"""
    x = np.array(x256, np.float64)
    x = x.reshape((4, 64) + x.shape[1:])
    o = 32
    while o:
        x[:, :o] = x[:, :o] + x[:, o:2 * o]
        o >>= 1
    return ((x[0, 0] + x[1, 0]) + x[2, 0]) + x[3, 0]


def _strided(x, width):
    """[n, ...] -> [width, ...]: slot k adds rows k, k + width, .. ascending, from 0.0"""
    x = np.asarray(x, np.float64)
    rounds = -(-len(x) // width)
    pad = np.zeros((rounds * width,) + x.shape[1:])        # adding +0.0 changes no sum that began at +0.0
    pad[:len(x)] = x
    acc = np.zeros((width,) + x.shape[1:])
    for r in pad.reshape((rounds, width) + x.shape[1:]):
        acc = acc + r
    return acc


def grid_stride_record(terms, max_blocks=None):
    """terms [n, ...] -> partials [blocks, ...], blocks = min(ceil(n / 256), max_blocks): thread (b, t) adds the elements
    b * 256 + t, + blocks * 256, .. ascending from 0.0, then block_sum per block"""
    x = np.asarray(terms, np.float64)
    blocks = -(-len(x) // 256)
    if max_blocks is not None:
        blocks = min(blocks, max_blocks)
    if blocks == 0:
        return np.zeros((0,) + x.shape[1:])
    acc = _strided(x, blocks * 256).reshape((blocks, 256) + x.shape[1:])
    return np.stack([block_sum(a) for a in acc])


def close_strided(partials, max_mask=0):
    """partials [nPart, width] (or [nPart]) -> [width]: reduce_partials_kernel.  Bit v of max_mask: column v is the largest
    partial (from 0.0) instead of the sum -- a maximum has no order to model."""
    p = np.asarray(partials, np.float64)
    out = block_sum(_strided(p, 256))
    for v in range(p.shape[1] if p.ndim > 1 else 0):
        if max_mask >> v & 1:
            out[v] = max(0.0, p[:, v].max()) if len(p) else 0.0
    return out


def close_serial(partials):
    """partials [nPart, width] -> [width]: pose_close_kernel, t = 0.0; t += part[b] for b ascending"""
    p = np.asarray(partials, np.float64)
    t = np.zeros(p.shape[1:])
    for row in p:
        t = t + row
    return t


def ordered_sum(values):
    """one value per thread, a block per 256, closed by close_strided: dist_sum of isdf_nn_distance, record[0] of isdf_tri_distance"""
    return float(close_strided(grid_stride_record(values)))


def wide(rng, shape, lo=-20, hi=20):
    """float32 values of either sign whose magnitudes spread evenly over 2^lo .. 2^hi: sums of them depend on the order"""
    return (rng.choice([-1.0, 1.0], shape) * np.exp2(rng.uniform(lo, hi, shape))).astype(np.float32)
