from equiadapt_amd.nbody.canonicalization_networks import custom_equivariant_networks, custom_group_equivariant_layers  # noqa: F401
from equiadapt_amd.nbody.canonicalization_networks.custom_equivariant_networks import (  # noqa: F401
    SequentialMultiple,
    VNDeepSetLayer,
    VNDeepSets,
)
from equiadapt_amd.nbody.canonicalization_networks.custom_group_equivariant_layers import VNLeakyReLU, VNSoftplus  # noqa: F401
