"""Test-side backend of a chain IcpFarm worker (farm.IcpFarm(chain, _backend="farm_chain_backend:oracle_chain_compute")):
the (name, run) contract of farm._hip_compute on the CPU.  The worker receives ``IcpChain.as_dict()``, rebuilds the
chain, filters every cloud with tests/dpf_ref.py (octree stages: the oracle's downsample) and runs the oracle on the
filtered clouds -- the numpy restatement of tests/icp_chain_ref.py when the chain lists outlier filters or the Bound
checker.  Test infrastructure only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DPF_EMPTY = 7   # SFE_ICP_DPF_EMPTY


def chain_job(chain, src, tgt, guess):
    """one job of a chain on the CPU -> (status, T 3 x 3 float32, iterations)"""
    import numpy as np

    import dpf_ref
    import icp_chain_ref
    import oracle
    s = dpf_ref.apply(src, chain.reading, oracle.downsample)
    t = dpf_ref.apply(tgt, chain.reference, oracle.downsample)
    if len(s) == 0 or len(t) == 0:
        return DPF_EMPTY, np.asarray(guess, np.float32).reshape(3, 3).copy(), 0
    if chain.outliers.any():
        return icp_chain_ref.icp(s, t, guess, chain.params, chain.outliers)
    return oracle.icp(s, t, np.asarray(guess, np.float32).reshape(3, 3),
                      oracle.IcpParams(precision=1, **chain.params.as_dict()))


def oracle_chain_compute(device, params_dict):
    from sonar_slam_amd import farm, icp_config
    if not farm.is_chain_dict(params_dict):
        raise TypeError("oracle_chain_compute: a chain farm hands over IcpChain.as_dict(), got %r" % sorted(params_dict))
    chain = icp_config.IcpChain.from_dict(params_dict)

    def run(v, chunk):
        for j, (s0, ns, t0, nt) in enumerate(v["jobs4"]):
            st, T, it = chain_job(chain, v["src"][s0:s0 + ns], v["tgt"][t0:t0 + nt], v["guess"][j])
            v["status"][j], v["T"][j], v["iters"][j] = st, T, it
    return "oracle chain worker %d (pid %d)" % (device, os.getpid()), run
