"""Child process of tests/test_gpu_light_shapes.py::test_k_light_branches_ran (not a test module).

Started with RDFIND_HIP_LIB = the instrumented variant of the library, RDFIND_LIGHT_DUMP = a file of its own and the
switches of one family in the environment; runs the named shapes (plain form, projection s, strategy 1, clean) and
prints one ``STATS {json}`` line per shape: the result's count and checksum, and sums over the per-item records of
k_light (kernels.inl RDF_LIGHT_STATS; the layout is tools/light_items.py NAMES)."""
import json
import os
import sys

import numpy as np

from rdfind_amd import _lib
from tests import light_shapes as L
from tools.light_items import NAMES, RECORD_WORDS


def main(names):
    dump = os.environ["RDFIND_LIGHT_DUMP"]
    with _lib.Context(0) as ctx:
        for name in names:
            sh = L.shape(name)
            if os.path.exists(dump):
                os.remove(dump)
            ctx.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
            ctx.run(sh.min_support, "s", True, 1)
            r = np.fromfile(dump, dtype=np.uint32).reshape(-1, RECORD_WORDS).astype(np.int64) if os.path.exists(dump) \
                else np.zeros((0, RECORD_WORDS), np.int64)
            col = {n: r[:, i] for i, n in enumerate(NAMES)}
            out = {"shape": name, "n_cinds": ctx.cind_count(), "checksum": ctx.checksum(), "items": int(r.shape[0]),
                   "max_nseg": int(col["nseg"].max(initial=0)), "win": int(col["win"].sum()),
                   "ser": int((col["ser"] & 0xFFFF).sum()), "sweep": int((col["ser"] >> 16).sum()),
                   "bat": int(col["bat"].sum()), "dser": int(col["dser"].sum()), "rows": int(col["rows"].sum()),
                   "killed_in_window": int(((col["alive1"] > 0) & (col["alive1"] < col["alive0"]) & (col["win"] > 0)).sum())}
            print("STATS " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
