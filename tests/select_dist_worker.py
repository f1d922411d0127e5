"""Worker of tests/test_gpu_select.py::test_one_rank_torch_world_gives_the_single_gpu_frame: one rank of an RCCL ("nccl")
world, launched by ``python -m torch.distributed.run``.  ``fit(min_similarity=t, world=TorchWorld(loop="c"))`` runs the
sharded C loop; each rank selects its own columns and rank 0 merges the pieces: the frame must be the single GPU's."""
import os
import sys

import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
    import simrank_amd.SimRank as SRA
    from simrank_amd import synth
    from simrank_amd.driver import TorchWorld
    from tests.graphs import bipartite_random
    from tests.test_gpu_select import assert_near, dense_pairs
    rank = dist.get_rank()
    df = synth.powerlaw_directed(600, 6, seed=17)
    for cls in ("SimRank", "SimRankPP"):
        dense = getattr(SRA, cls)().fit(df, verbose=False, world=TorchWorld(loop="c", handback="all"))
        for t in (0.01, 0.05):
            one = getattr(SRA, cls)().fit(df, verbose=False, min_similarity=t)
            want = dense_pairs(dense, t)
            for handback in ("root", "all"):
                got = getattr(SRA, cls)().fit(df, verbose=False, min_similarity=t,
                                              world=TorchWorld(loop="c", handback=handback))
                if rank == 0 or handback == "all":
                    pd.testing.assert_frame_equal(got, want, check_exact=True)
                    assert_near(got, one, t)
                    assert len(got) > 0
                else:
                    assert got is None
    dfb = bipartite_random(170, 90, 0.06, seed=22)
    d1, d2 = SRA.BipartiteSimRankPP().fit(dfb, verbose=False, strict_reference=False,
                                          world=TorchWorld(loop="c", handback="all"))
    got = SRA.BipartiteSimRankPP().fit(dfb, verbose=False, strict_reference=False, min_similarity=0.02,
                                       world=TorchWorld(loop="c", handback="all"))
    for a, d in zip(got, (d1, d2)):
        pd.testing.assert_frame_equal(a, dense_pairs(d, 0.02), check_exact=True)
    # the max_pairs refusal reaches every rank alike
    try:
        SRA.SimRank().fit(df, verbose=False, min_similarity=0.01, max_pairs=1, world=TorchWorld(loop="c"))
        raise AssertionError("max_pairs was not enforced")
    except ValueError as e:
        assert "max_pairs=1" in str(e)
    dist.barrier()
    dist.destroy_process_group()
    print("SELECT WORLD ok", rank)


if __name__ == "__main__":
    main()
