"""
The swarm alone against the replica's minimiser (tests/test_gpu_calibration.py): every study of
tests/calibration_support.py's device cases at pyswarm's default stopping rule, at swarm sizes 64 and 204 -- how far the
swarm stops from the polished fit in standard errors, and what that does to ``params_std`` and ``area_fraction_std``
against the spread of the linear predictions.  Also the worst |D_k - D_lin,k| / sigma_x of the polished fits beside the
host reference's.

    python tools/replica_calibration.py > profiles/rNN/replica_calibration.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import calibration_support as C                      # noqa: E402
from tests import test_gpu_calibration as G                      # noqa: E402


def main():
    print("replica calibration: polished fits against the linear response of their own noise")
    print("(sigma_x: the sandwich standard error of the host truth; bar: twice the host reference's remainder + stop)")
    for name in G.DEVICE_CASES:
        c = C.case(name)
        for S in (64, 204):
            s = G.run_study(c, swarmsize=S)
            t = s["truth"]
            pw = C.pointwise(t, s["polished"][1:] - t.x0)
            print("%s, swarmsize %d: N %d, P %d, M %d, sigma_v / sigma_u %g; %.2f s; polish %d launches, stops %s"
                  % (name, S, c.N, c.P, c.M, c.ratio, s["seconds"], s["info"]["launches"], sorted(set(s["info"]["stop"]))))
            print("    polished: worst |D_k - D_lin,k| / sigma_x %.4f (host TRF %.4f, bar %.4f)"
                  % (pw.max(), C.REMAINDER_MEASURED[c.key], C.bar(c)))
            print("    " + G.swarm_report(s, "swarm alone:"))
            dist, infl, af = G.swarm_alone(s)
            print("    params_std inflation per parameter: %s" % np.round(infl, 3))


if __name__ == "__main__":
    main()
