"""vtkcloudpoint_amd -- MI355X-native DBSCAN + centroid + ICP hot path of ZhiHuangHn/vtkCloudPoint.

The compute lives in libvcp.so (hand-written HIP for gfx950 behind the C-ABI of include/vcp.h);
this package is the thin host-side mirror of the reference's class surface.
"""
__version__ = "0.1.0"


_LAZY = {
    "cluster_quantiles": "robust", "cluster_medians": "robust", "cluster_mad": "robust", "robust_fixed_centroids": "robust",
    "cluster_moments": "moments", "ellipse_radius": "moments", "ellipse_sides": "moments", "filter_by_moments": "moments",
    "ClusterMoments": "moments",
    "cluster_spheres": "spheres", "sphere_centres": "spheres", "filter_by_spheres": "spheres", "ClusterSpheres": "spheres",
    "extract_planes": "planes", "plane_score": "planes", "planes_from_triples": "planes", "plane_label": "planes",
    "plane_residuals": "planes", "remove_planes": "planes", "plane_score_shape": "planes", "Planes": "planes",
    "point_features": "features", "sor_keep": "features", "centre_votes": "features", "point_features_shape": "features",
    "PointFeatures": "features",
}


def __getattr__(name):
    """The per-cluster statistics, the plane extraction and the per-point features by name (robust.py, moments.py,
    spheres.py, planes.py, features.py), imported on first use: importing the package loads neither numpy nor the library."""
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
