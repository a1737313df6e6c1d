"""BigCLAM compute ops.

``reference``: vectorized torch implementations (CPU path + numerics
reference).  ``hip``: hand-written CDNA4 HIP kernels (GPU path; requires the
in-tree ``bigclam._C`` extension built for gfx950).  ``cover_cpu``: the
vectorised CPU best-match between two covers (CPU path + oracle of K8) and
per-community edge counts of a cover on a graph (CPU path + oracle of K10).
``links_cpu``: top-n link recommendation from the sparse model (CPU path +
oracle of K11).
"""
from . import reference  # noqa: F401
