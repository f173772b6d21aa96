"""`simple_knn._C` of the reference (submodules/simple-knn/ext.cpp: distCUDA2), re-exported from the
package's extension."""
from relightable3dgaussian_amd.simple_knn import distCUDA2  # noqa: F401
