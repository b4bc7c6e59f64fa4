"""Seed derivation for batch-invariant (``per_item``) sampling: host-side integer arithmetic only.

A sampling run has one 64-bit ``seed``; every item gets its own 64-bit Philox seed derived from it and from a key that names the
item independently of the batch it rides in - its index in the call, or ``path_key`` of its file's path relative to the data
folder - and every window of a chunked item one derived from the item's.  The mixing step is SplitMix64 (Steele, Lea & Flood,
"Fast splittable pseudorandom number generators", OOPSLA 2014; the seeding generator of java.util.SplittableRandom and xoshiro).
"""
from __future__ import annotations

import hashlib

MASK64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    """One SplitMix64 step: the output for state ``x`` (the state is advanced by the golden-ratio increment, then mixed)."""
    z = (int(x) + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def item_seed(seed: int, key: int) -> int:
    """The Philox seed of the item named ``key`` (an integer: its index, or ``path_key``) in the run seeded ``seed``."""
    return splitmix64((int(seed) & MASK64) ^ splitmix64(int(key) & MASK64))


def path_key(rel_path) -> int:
    """A 64-bit key of a file: the first 8 bytes, little endian, of BLAKE2b over the POSIX-style relative path in UTF-8
    (backslashes count as separators, so that one data set gives the same keys on every OS)."""
    posix = str(rel_path).replace("\\", "/")
    return int.from_bytes(hashlib.blake2b(posix.encode("utf-8")).digest()[:8], "little")


def window_seed(item_seed_: int, k: int) -> int:
    """The Philox seed of window ``k`` of a chunked item."""
    return splitmix64((int(item_seed_) + int(k) + 1) & MASK64)


def item_seeds(seed: int, n: int):
    """``[item_seed(seed, b) for b in range(n)]``: the default when a per-item run names no seeds."""
    return [item_seed(seed, b) for b in range(int(n))]
