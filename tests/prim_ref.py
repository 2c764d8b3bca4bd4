"""NumPy references of the device primitives in rdfind_amd/csrc/primitives.hip (pure NumPy, no GPU):
the exclusive scans and the stable LSD radix sort / partition family.  tests/test_prim_ref.py checks these against
plain Python; tests/test_gpu_primitives.py compares the HIP kernels with them element for element."""
import numpy as np

M64 = (1 << 64) - 1
PAD = np.uint64(M64)  # the padding key radix_sort_u64_drop leaves out


def exclusive_scan(values, out_dtype):
    """(out, total): out[i] = sum(values[:i]), total = sum(values), accumulated in uint64 and reduced to
    ``out_dtype`` (uint32: modulo 2^32, the defined unsigned wrap of the u32 -> u32 scan)."""
    v = np.asarray(values).astype(np.uint64)
    incl = np.cumsum(v, dtype=np.uint64)
    out = np.zeros(v.shape[0], np.uint64)
    out[1:] = incl[:-1]
    total = int(incl[-1]) if v.shape[0] else 0
    if np.dtype(out_dtype) == np.uint32:
        return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32), total & 0xFFFFFFFF
    return out, total


def mix64(x):
    """common.hpp mix64 (murmur3 finaliser) on a uint64 array (the products wrap modulo 2^64)."""
    x = np.asarray(x, dtype=np.uint64).copy()
    s = np.uint64(33)
    x ^= x >> s
    x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> s
    x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> s
    return x


def bit_field(keys, lo, hi):
    """Bits [lo, hi) of each key, as uint64 (hi <= lo: all zero)."""
    k = np.asarray(keys).astype(np.uint64)
    if hi <= lo:
        return np.zeros(k.shape[0], np.uint64)
    width = hi - lo
    mask = np.uint64(M64 if width >= 64 else (1 << width) - 1)
    return (k >> np.uint64(lo)) & mask


def stable_by(keys, field):
    """``keys`` in ascending order of ``field``, ties in input order."""
    keys = np.asarray(keys)
    field = np.asarray(field)
    if field.size and int(field.max()) < (1 << 16):  # (same order; NumPy sorts 16-bit integers by radix, much faster)
        field = field.astype(np.uint16)
    return keys[np.argsort(field, kind="stable")]


def sort_bits(keys, lo, hi):
    """radix_sort_u64_bits / radix_partition_u32: stable on bits [lo, hi) (hi <= lo: the identity)."""
    return stable_by(keys, bit_field(keys, lo, hi))


def sort_drop(keys, bits):
    """radix_sort_u64_drop: the keys other than ~0, stable on the low ``bits`` bits; its length is n_out."""
    k = np.asarray(keys, dtype=np.uint64)
    k = k[k != PAD]
    return stable_by(k, bit_field(k, 0, bits))


def partition_hashed(keys, bits, hmask):
    """radix_partition_hashed: stable on the top ``bits`` bits of mix64(key & hmask)."""
    k = np.asarray(keys, dtype=np.uint64)
    return stable_by(k, mix64(k & np.uint64(hmask & M64)) >> np.uint64(64 - bits))
