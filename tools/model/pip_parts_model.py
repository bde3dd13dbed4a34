#!/usr/bin/env python3
"""Wavefront-level cost model of the Pippenger bucket stage (k_pip_bucket_part + k_pip_bucket_merge) for the flagship shape: one batch of
4,096 CMZ proofs, c = 11 -- 24 windows of 1,024 buckets, 431 bucket entries per proof, Poisson bucket sizes.

A wavefront costs what its LONGEST lane costs, so the model packs the parts (virtual lanes, in bucket order as k_pip_vmap lays them out)
into wavefronts of 64 and sums each wavefront's maximum, in field multiplications: 7 per mixed addition, 9 per merge addition of a lane
(ge_to_cached + ge_add_cached), 4.5 per quad lane and merge addition (four lanes at about half an addition each, quad.h), 1.3 for
ge_from_niels.  It answers three questions of the round-8 change without a GPU:

  * what a chain that starts AT its first entry saves in k_pip_bucket_part (one addition per part: the longest lane too);
  * whether parts of equal length (len = cnt / parts, +1 for the first cnt mod parts) instead of (L, L, ..., remainder) save anything:
    they do not -- the lanes that go idle sit in wavefronts whose longest lane still runs L entries;
  * which part length a many-batch call should use once the merge runs one lane per bucket: 16, 32, 64 or whole buckets.

    python tools/model/pip_parts_model.py [seed]
"""
import sys

import numpy as np

M_MADD, M_MERGE_LANE, M_MERGE_QUAD, M_FROM_NIELS = 7.0, 9.0, 4.5, 1.3


def wave_max_sum(a):
    a = np.asarray(a)
    a = np.concatenate([a, np.zeros((-len(a)) % 64, a.dtype)]).reshape(-1, 64)
    return int(a.max(1).sum())


def split(cnt, L, balanced):
    """part lengths of a bucket of cnt entries (part_len / part_count of zkp_kernels.hip; balanced = the variant that was not kept)"""
    if cnt == 0:
        return []
    pl = max(L, min(4 * L, int(np.ceil(np.sqrt(cnt)))))
    parts = -(-cnt // pl)
    if balanced:
        q, r = divmod(cnt, parts)
        return [q + (i < r) for i in range(parts)]
    return [min(pl, cnt - i * pl) for i in range(parts)]


def main():
    rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
    cnt = rng.poisson(4096 * 431 / 24 / 1024, size=4 * 24 * 1024)           # four batches' worth of buckets
    print("%-14s %-9s %8s %12s %12s %12s %12s %12s" % ("part length", "split", "parts", "part, id+e", "part, first", "merge quad", "merge lane", "first+lane"))
    for L in (16, 32, 64, 1 << 30):
        for balanced in (False, True):
            lens, nparts = [], []
            for c in cnt:
                p = split(int(c), L, balanced)
                lens += p
                nparts.append(len(p))
            lens, nparts = np.array(lens), np.array(nparts)
            ident = wave_max_sum(lens) * M_MADD                                          # identity + entry: every entry is an addition
            first = wave_max_sum(lens - 1) * M_MADD + (len(lens) / 64) * M_FROM_NIELS     # the first entry is the accumulator
            mq = wave_max_sum(np.repeat(np.maximum(nparts - 1, 0), 4)) * M_MERGE_QUAD
            ml = wave_max_sum(np.maximum(nparts - 1, 0)) * M_MERGE_LANE
            print("%-14s %-9s %8d %12.0f %12.0f %12.0f %12.0f %12.0f" % ("whole bucket" if L > 64 else L, "balanced" if balanced else "L + rest", len(lens), ident, first, mq, ml,
                                                                           first + ml))


if __name__ == "__main__":
    main()
