"""One process with SYLPH_HIP_HIT_SORT set (the switch is read once per process): the sorted finish of contain.hip — pack or keep the hit
keys, radix sort, offsets by binary search, narrow — on ORDINARY inputs, which otherwise reach it only through a count of 4096 and
above.  The ladder cases, the row-count edges (without the two 65k-genome databases) and the 9- and 64-table batches of
tests/contain_edges.py against the expectation by construction and the oracle; every call with hits must have sorted and none may have
run the row assembly.  Started by tests/test_gpu_contain_edges.py."""
import os
import sys

import numpy as np

import sylph_amd as S

from . import contain_edges as E


def main():
    assert os.environ.get("SYLPH_HIP_HIT_SORT"), "start me with SYLPH_HIP_HIT_SORT set"
    import torch                                                 # (device-resident tables; torch brings its runtime up first)
    torch.cuda.init()
    ctx = S.Context(0)
    ctx.profile(True)
    # a. rows and values: one database per distinct key set (the 16 batch-maximum cases share theirs)
    by_db = {}
    for name, build in E.ladder_cases().items():
        case = build()
        by_db.setdefault(case.db_kmers.tobytes(), []).append((name, case))
    assert len(by_db) == len(E.PATTERNS) + 2
    for cases in by_db.values():
        db = S.Database(ctx, cases[0][1].db_kmers, cases[0][1].goff)
        for name, case in cases:
            E.assert_oracle(case, 0.0)
            mx = E.hit_max(case)
            assert E.check_single(ctx, db, case, 0.0, forced=True) == (np.uint8 if mx <= 255 else np.uint16 if mx <= 65535 else np.uint32), name
        db.close()
    # b. row counts: G and 3 G rows
    for G in E.TINY_G:
        if G >= 65535:
            continue
        db_kmers, goff, _ = E.tiny_db(G)
        singles = [E.tiny_case(G, v) for v in (0, 1, 2)]
        db = S.Database(ctx, db_kmers, goff)
        for case in singles:
            E.assert_oracle(case, 0.0)
            assert E.check_single(ctx, db, case, 0.0, forced=True) == np.uint8
        assert E.check_batch(ctx, db, E.stack_cases(singles), 0.0, forced=True, device=False) == np.uint8
        db.close()
    # c. batches of 9 and 64 tables, host and device resident, every slice against its single-sample call
    db_kmers, goff = E.batch_db()[3:]
    db = S.Database(ctx, db_kmers, goff)
    for n_tables in (9, 64):
        for kind in ("mixed", "wide", "empty") if n_tables == 9 else ("mixed", "wide"):
            case = E.batch_case(n_tables, kind)
            E.assert_oracle(case, E.BATCH_MIN_KMERS)
            E.check_batch(ctx, db, case, E.BATCH_MIN_KMERS, forced=True, singles=kind == "mixed")
    db.close()
    ctx.profile(False)
    ctx.close()
    print("contain edges sorted ok")


if __name__ == "__main__":
    sys.exit(main())
