"""Drop-in replacement for the reference's compiled `simple_knn` package (submodules/simple-knn,
ext `simple_knn._C`: distCUDA2, submodules/simple-knn/ext.cpp).

With `integration/` on PYTHONPATH this reference import resolves to the MI355X build unchanged:
    scene/gaussian_model.py:13        from simple_knn._C import distCUDA2
"""
from relightable3dgaussian_amd.simple_knn import distCUDA2  # noqa: F401  (ImportError if the HIP build is missing)
