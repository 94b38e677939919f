from .uipc_sim import UipcSim, UipcSimCfg
from .uipc_object import GelMaterialCfg, UipcObject, UipcObjectCfg
from .uipc_attachments import UipcIsaacAttachments, UipcIsaacAttachmentsCfg

__all__ = ["UipcSim", "UipcSimCfg", "UipcObject", "UipcObjectCfg", "GelMaterialCfg", "UipcIsaacAttachments", "UipcIsaacAttachmentsCfg"]
