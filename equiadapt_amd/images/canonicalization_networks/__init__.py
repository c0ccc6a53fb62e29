from equiadapt_amd.images.canonicalization_networks.custom_equivariant_networks import CustomEquivariantNetwork  # noqa: F401
from equiadapt_amd.images.canonicalization_networks.custom_group_equivariant_layers import (  # noqa: F401
    RotationEquivariantConv,
    RotationEquivariantConvLift,
    RotoReflectionEquivariantConv,
    RotoReflectionEquivariantConvLift,
)
from equiadapt_amd.images.canonicalization_networks.custom_nonequivariant_networks import (  # noqa: F401
    ConvNetwork,
    ResNet18Network,
    WideResNet50Network,
    WideResNet101Network,
)
from equiadapt_amd.images.canonicalization_networks.escnn_networks import (  # noqa: F401
    ESCNNEquivariantNetwork,
    ESCNNSteerableNetwork,
    ESCNNWideBasic,
    ESCNNWideBottleneck,
    ESCNNWRNEquivariantNetwork,
)
from equiadapt_amd.images.canonicalization_networks import (  # noqa: E402,F401  (submodule aliases, equiadapt/images/__init__.py)
    custom_equivariant_networks,
    custom_group_equivariant_layers,
    custom_nonequivariant_networks,
    escnn_networks,
)
