"""Backbone names (reference code/yolo3/enums.py:25-28), box-loss kinds (:32-34) and data set modes (:38-41)."""
from enum import Enum, unique


@unique
class BACKBONE(Enum):
    MOBILENETV2x75 = 0
    MOBILENETV2x14 = 1
    EFFICIENTNETB3 = 2


@unique
class BOX_LOSS(Enum):
    MSE = 0
    GIOU = 1


@unique
class DATASET_MODE(Enum):
    TRAIN = 0
    VALIDATE = 1
    TEST = 2
