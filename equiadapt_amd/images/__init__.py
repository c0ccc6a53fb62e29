from equiadapt_amd.images.canonicalization_networks.custom_nonequivariant_networks import (  # noqa: F401
    WideResNet50Network,
    WideResNet101Network,
)
