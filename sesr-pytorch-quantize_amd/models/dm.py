"""DM demosaic net (MFLAG 2): 3 -> 16 -> ... -> 3 channels, no upscaling -- the class body of nrdm_3_sim (reference models/dm.py).

The reference's dm.dm() keeps the long skip as a float AddOp; its integer net is the nrdm_3_sim graph with this task's weights and
domains, the skip merged in the integer domain as for MFLAG 3."""
from models.model_utils_pt import CollapsibleNet


class dm(CollapsibleNet):
    def __init__(self, in_channels=3, out_channels=3, num_channels=16, num_lblocks=3, scaling_factor=1):
        super().__init__(in_channels, out_channels, num_channels, num_lblocks, scaling_factor)
