"""EigenPlaces global-descriptor plugin on the MI355X HIP backend (extractor conf `eigenplaces`).

Drop-in for imcui/hloc/extractors/eigenplaces.py: same module name, one BaseModel subclass `EigenPlaces`, same `default_conf` (:33-37),
`required_inputs` (:38) and output (:56-58).  The architecture is CosPlace's (upstream's EigenPlaces copies its network.py), so the class
is the CosPlace plugin with the other hub repository and checkpoint suffix; conf["variant"] may also name "CosPlace", as the reference
allows (:42).  Everything cosplace.py here says about what is restated and what is unverified holds for this plugin too.
"""
from __future__ import annotations

from .cosplace import CosPlace


class EigenPlaces(CosPlace):
    default_conf = {"variant": "EigenPlaces", "backbone": "ResNet101", "fc_output_dim": 2048}
    required_inputs = ["image"]

    def _init(self, conf):
        if conf["variant"] not in ("EigenPlaces", "CosPlace"):
            raise ValueError(f"eigenplaces: unknown variant {conf['variant']!r} (EigenPlaces or CosPlace)")
        self.variant = conf["variant"]
        super()._init(conf)
