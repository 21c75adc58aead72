"""One rank of the world-size-2 test of api.stability_check (gloo, CPU, stand-in repeat runner)."""
import argparse
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch.distributed as dist  # noqa: E402

from resnmtf_amd import api  # noqa: E402
from stability_ref import fake_results, fake_runner  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rank", type=int); ap.add_argument("--world", type=int); ap.add_argument("--port", type=int)
ap.add_argument("--out")
a = ap.parse_args()
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{a.port}", rank=a.rank, world_size=a.world)
results, data = fake_results()
runner = fake_runner(n_views=2, k=4)
out = api.stability_check(data, results, 4, None, None, None, 20, False, 5, False, "euclidean", n_stability=7,
                          stab_thres=0.5, remove_unstable=False, repeat_runner=runner)
kept = api.stability_check(data, results, 4, None, None, None, 20, False, 5, False, "euclidean", n_stability=7,
                           stab_thres=0.5, repeat_runner=runner)
if a.rank == 0:
    pickle.dump({"relevance": out["relevance"], "row_clusters": kept["row_clusters"],
                 "col_clusters": kept["col_clusters"]}, open(a.out, "wb"))
dist.barrier()
dist.destroy_process_group()
