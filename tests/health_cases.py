"""Shared inputs of the flight-recorder tests (test_health_rule_cpu.py, test_health_gpu.py): the segment lengths at which the rule
can go wrong -- vector heads and tails, the 256-lane and 1024-element rows, the 16384-element block boundary, a multi-block fold --
and the values that have to be classified exactly, planted at the first and last element and on both sides of a block boundary."""
import numpy as np

BLOCK = 16384
LENGTHS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 3 * 16384 + 5]
# fp32 bit patterns: NaN, +inf, -inf, smallest and largest denormal, -0.0, FLT_MAX, -FLT_MAX
SPECIAL32 = {'nan': 0x7fc00000, 'pinf': 0x7f800000, 'ninf': 0xff800000, 'den_min': 0x00000001, 'den_max': 0x807fffff, 'nzero': 0x80000000,
             'fltmax': 0x7f7fffff, 'nfltmax': 0xff7fffff}
VARIANTS = ['plain'] + list(SPECIAL32) + ['mixed']


def plant_positions(n):
    """first and last element, both sides of every block boundary inside the segment"""
    pos = {0, n - 1}
    for b in range(BLOCK, n + 1, BLOCK):
        pos |= {b - 1, b}
    return sorted(p for p in pos if 0 <= p < n)


def make_bits(n, bf16, variant, seed):
    """the raw bit patterns (uint32, or uint16 for bf16) of a random finite segment of n elements with `variant` planted"""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal(n) * np.exp(rs.uniform(-6, 6, n))).astype(np.float32)
    x[rs.rand(n) < 0.05] = 0.0                                   # some exact zeros
    bits = x.view(np.uint32).copy()
    if variant != 'plain':
        names = list(SPECIAL32)
        for k, p in enumerate(plant_positions(n)):
            bits[p] = SPECIAL32[variant] if variant != 'mixed' else SPECIAL32[names[(k + seed) % len(names)]]
    if bf16:
        return (bits >> 16).astype(np.uint16)                   # truncation keeps every class (NaN stays NaN, a denormal stays one or 0)
    return bits


def widen(bits):
    """bit patterns -> float32 values (bf16 widened exactly)"""
    if bits.dtype == np.uint16:
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return bits.view(np.float32)
