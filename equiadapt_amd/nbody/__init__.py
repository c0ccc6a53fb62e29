from equiadapt_amd.nbody.canonicalization.euclidean_group import EuclideanGroupNBody  # noqa: F401
from equiadapt_amd.nbody.canonicalization_networks import VNDeepSets  # noqa: F401
from equiadapt_amd.nbody.graph import complete_graph_edges  # noqa: F401
