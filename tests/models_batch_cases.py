"""The batches tests/test_gpu_models_batch.py draws on the device, with their restated twins (tests/models_batch_oracle.py).  The host
test checks on the CPU that the restatement's ill-conditioned blocks stay a negligible share of every batch."""
import functools

from tests import models_batch_oracle as O

GAP_MIN = 1e-2           # blocks whose restated gap is below this are left out of the comparison with LAPACK's SVD


def _uni(n, p, seed, q=0.3, sigma=0.1, model="uniform"):
    return dict(n=n, p=p, q=q, sigma=sigma, model=model, seed=seed)


def _non(n, p, seed, crpt_type, p_node_crpt=1.0, p_edge_crpt=1.0, sigma_in=0.1, sigma_out=0.2):
    return dict(n=n, p=p, p_node_crpt=p_node_crpt, p_edge_crpt=p_edge_crpt, sigma_in=sigma_in, sigma_out=sigma_out, crpt_type=crpt_type, seed=seed)


MODELS = ("uniform", "self-consistent")
UNIFORM = {
    "tiny": [_uni(2, 0.7, 11), _uni(3, 0.7, 12, model="self-consistent"), _uni(2, 1.0, 13)],
    "wave": [_uni(64, 0.5, 21), _uni(65, 0.5, 22, model="self-consistent"), _uni(129, 0.4, 23)],      # a row ends at, one past, two past a wave
    "none": [_uni(12, 0.0, 31)],
    "complete": [_uni(12, 1.0, 41, model="self-consistent"), _uni(65, 1.0, 42)],
    "mixed": [_uni(5, 0.5, 51), _uni(40, 0.5, 52, model="self-consistent"), _uni(129, 0.3, 53), _uni(12, 0.0, 54), _uni(65, 0.6, 55, q=0.5)],
    "one": [_uni(40, 0.5, 61, model="self-consistent")],
    "many": [_uni(8, 0.6, 1000 + b, model=MODELS[b % 2]) for b in range(300)],
    "q_edges": [_uni(20, 0.8, 71, q=0.0), _uni(20, 0.8, 72, q=1.0), _uni(20, 0.8, 73, q=1.0, model="self-consistent")],
}
NONUNIFORM = {
    # both endpoints select every edge: the winner rule decides every block
    "all": [_non(n, 1.0 if n == 12 else 0.5, 100 * n + t, ct) for n in (12, 65) for t, ct in enumerate(("uniform", "self-consistent", "adv"))],
    "partial": [_non(40, 0.5, 81, "adv", 0.3, 0.5), _non(40, 0.5, 82, "uniform", 0.25, 0.7), _non(10, 0.9, 83, "self-consistent", 0.25, 0.4),
                _non(30, 0.5, 84, "adv", 0.0, 1.0), _non(30, 0.5, 85, "adv", 1.0, 0.0)],
    # more nodes than the selection kernel stages at a time: its strided path
    "long_rows": [_non(1030, 0.01, 91, "adv", 0.02, 0.5)],
}


def columns(specs):
    """The keyword arguments of a *_Topology_batch call from a list of per-problem dicts."""
    names = [k for k in specs[0] if k != "seed"]
    kw = {k: [s[k] for s in specs] for k in names}
    kw["seeds"] = [s["seed"] for s in specs]
    return kw


@functools.lru_cache(maxsize=None)
def restated(kind, name):
    """The restated problems of a batch, computed once and shared by the tests (treat as read-only)."""
    if kind == "uniform":
        return tuple(O.uniform_topology(**s) for s in UNIFORM[name])
    return tuple(O.nonuniform_topology(**s) for s in NONUNIFORM[name])
