from .sod_metrics import (  # noqa: F401
    SodMetricSet,
    TFEmeasureMetric,
    TFFmeasureMetric,
    TFMAEMetric,
    TFSmeasureMetric,
    TFWeightedFmeasureMetric,
)
