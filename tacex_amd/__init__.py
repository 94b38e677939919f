"""tacex_amd - MI355X-native GelSight tactile-image engine behind TacEx's sensor / simulator plugin API."""
from .camera_model import CameraProfile, TactileCameraModel
from .contact_field import ContactField, ContactGel, PartContactField, TactileContactModel, slip_from_fots
from .contact_points import ContactPoints, TactileContactPoints
from .gel_memory import GelMemoryProfile, TactileGelMemory
from .gelsight_sensor import GelSightSensor
from .gelsight_sensor_cfg import GelSightSensorCfg
from .gelsight_sensor_data import GelSightSensorData
from .gelsight_sensor_group import GelSightSensorGroup
from .height_map_source import AffineBodyDepthSource, FemSurfaceDepthSource, FemTractionImage, IndenterHeightMapSource, MeshDepthSource, MeshLibraryDepthSource
from .lens_model import LensProfile, TactileLensModel
from .relief_source import ReliefHeightMapSource, ReliefTile
from .sdf_scene import SdfSceneSource, part_slip
from .volume_source import SdfVolume, SdfVolumeSource

__all__ = ["AffineBodyDepthSource", "CameraProfile", "ContactField", "ContactGel", "ContactPoints", "GelMemoryProfile", "GelSightSensor", "GelSightSensorCfg", "GelSightSensorData", "GelSightSensorGroup", "FemSurfaceDepthSource", "FemTractionImage", "IndenterHeightMapSource", "LensProfile", "MeshDepthSource",
           "MeshLibraryDepthSource", "PartContactField", "ReliefHeightMapSource", "ReliefTile", "SdfSceneSource", "SdfVolume", "SdfVolumeSource", "TactileCameraModel", "TactileContactModel", "TactileContactPoints", "TactileGelMemory", "TactileLensModel", "part_slip", "slip_from_fots"]
