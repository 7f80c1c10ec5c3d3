"""Child process of tests/test_sitecat_gpu.py: the site-category calls of one partition, with whatever
PLLHIP_SITECAT_BLOCKS the parent put into the environment.  Usage: _sitecat_worker.py STATES RATE_CATS NSITES OUT.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pllhip_ctypes as pc                              # noqa: E402
from test_ancestral_exact import build_case, triples_of   # noqa: E402


def run(product, states, rate_cats, nsites):
    """every array the calls return for the triples of the case, by name; the sums twice"""
    out = {}
    with build_case(product, states, rate_cats, nsites, True, "ambiguous", mixture_pinv=[0.2, 0.1]) as inst:
        t = inst.tree
        out["kernel"] = np.frombuffer(product.lib.pllhip_partials_kernel_name(inst.p), dtype=np.uint8)
        for k, (node, other, m) in enumerate(triples_of(t)):
            with pc.SiteCat.edge(inst, node, t.scaler_of(node), other, t.scaler_of(other), m) as sc:
                out[f"A{k}"], out[f"B{k}"], out[f"c{k}"] = sc.table()
                for rep in range(2):
                    po = sc.posteriors(flags=pc.PLLHIP_SITECAT_POSTERIORS)
                    for f in ("rate", "category", "category_prob", "invariant_prob", "lnl", "posterior"):
                        out[f"{f}{k}"] = getattr(po, f)
                    out[f"expected{k}_{rep}"], out[f"loglh{k}_{rep}"] = po.expected, np.array(po.loglh)
                if np.isfinite(po.loglh):
                    for rep in range(2):
                        fit = sc.em_weights(1e-6, 5)
                        out[f"em_w{k}_{rep}"], out[f"em_l{k}_{rep}"] = fit.trail_weights, fit.trail_loglh
    return out


if __name__ == "__main__":
    states, rate_cats, nsites = (int(x) for x in sys.argv[1:4])
    np.savez(sys.argv[4], **run(pc.PllLib(pc.PRODUCT_LIB), states, rate_cats, nsites))
