"""Sampling the imager on a grid (mrcal/utils.py:268-437): sample_imager() is host numpy, sample_imager_unproject()
runs over unproject() (the GPU)."""
import numpy as np


def sample_imager(gridn_width, gridn_height, imager_width, imager_height):
    """Regularly-sampled pixel coordinates across the imager, (gridn_height,gridn_width,2): [0,0] = (0,0),
    [-1,-1] = (imager_width-1,imager_height-1). gridn_height=None: int(round(imager_height/imager_width*gridn_width))"""
    if gridn_height is None:
        gridn_height = int(round(imager_height/imager_width*gridn_width))
    w = np.linspace(0, imager_width  - 1, gridn_width)
    h = np.linspace(0, imager_height - 1, gridn_height)
    return np.ascontiguousarray(np.stack(np.meshgrid(w, h), axis=-1))


def sample_imager_unproject(gridn_width, gridn_height, imager_width, imager_height, lensmodel, intrinsics_data,
                            normalize=False):
    """(v, q): the grid q of sample_imager() and its unprojection v (gridn_height,gridn_width,3); with a list or tuple
    of lens models (and as many intrinsics) v is (Ncameras,gridn_height,gridn_width,3), all of the one grid"""
    from . import unproject
    grid = sample_imager(gridn_width, gridn_height, imager_width, imager_height)
    if isinstance(lensmodel, (list, tuple)):
        return np.array([unproject(grid, lensmodel[i], intrinsics_data[i], normalize=normalize)
                         for i in range(len(lensmodel))]), grid
    return unproject(grid, lensmodel, intrinsics_data, normalize=normalize), grid
