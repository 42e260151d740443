"""Host-language mirror of pkg/fanal/analyzer/secret (undistro/trivy @ 2024-12-20)
and of the analyzer group's per-file fan-out for it, batched into arenas for the
MI355X engine (include/tsg_analyzer.h).  Files resident in HBM are analyzed through
SecretAnalyzer.ClassifyDevice / AnalyzeDevice / AnalyzeDeviceAsync (PendingDeviceAnalyze), a tar
layer resident in HBM through IndexLayerDevice / AnalyzeLayerDevice (DeviceTarIndex)."""
from .secret import (XFORM_DROP, AnalysisInput, AnalysisResult, AnalyzerOptions, Collector, DeviceTarIndex,
                     ExtractPrintableBytes,
                     FileInfo, IsBinary, NewSecretAnalyzer, PendingDeviceAnalyze, SecretAnalyzer,
                     SecretScannerOption, StripCR, TypeSecret)

__all__ = ["AnalysisInput", "AnalysisResult", "AnalyzerOptions", "Collector", "DeviceTarIndex", "ExtractPrintableBytes",
           "FileInfo", "IsBinary", "NewSecretAnalyzer", "PendingDeviceAnalyze", "SecretAnalyzer",
           "SecretScannerOption", "StripCR", "TypeSecret", "XFORM_DROP"]
