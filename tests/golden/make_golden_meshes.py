"""Generates tests/golden/meshes/ from the REFERENCE's mesh assets (fluidlab/assets/meshes), for tests/test_mesh.py.

    python tests/golden/make_golden_meshes.py <reference checkout>

Data only: the raw and processed .obj files the tests read, xz-compressed byte for byte, and the occupancy grid and transform of
the reference's voxelized/duck-128.vox (a pickled trimesh VoxelGrid) as plain arrays, read straight from the pickle stream
(unpickling would need trimesh)."""
import lzma
import os
import pickletools
import sys

import numpy as np

RAW = ['duck.obj', 'plate.obj', 'cup.obj', 'stirrer.obj', 'glass.obj', 'glass_vis.obj', 'room.obj', 'board.obj']
PROCESSED = ['plate-plate.obj', 'cup-cup.obj', 'stirrer-stirrer.obj', 'glass-glass_vis.obj', 'room-room.obj', 'board-board.obj']
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'meshes')


def main(ref):
    src = os.path.join(ref, 'fluidlab', 'assets', 'meshes')
    for kind, names in (('raw', RAW), ('processed', PROCESSED)):
        os.makedirs(os.path.join(OUT, kind), exist_ok=True)
        for name in names:
            with open(os.path.join(src, kind, name), 'rb') as fh:
                data = fh.read()
            with open(os.path.join(OUT, kind, name + '.xz'), 'wb') as fh:
                fh.write(lzma.compress(data, preset=9 | lzma.PRESET_EXTREME))
    with open(os.path.join(src, 'voxelized', 'duck-128.vox'), 'rb') as fh:
        stream = fh.read()
    blobs = [arg for op, arg, pos in pickletools.genops(stream) if op.name in ('BINBYTES', 'SHORT_BINBYTES') and len(arg) > 100]
    occ = np.frombuffer(blobs[0], dtype=np.bool_).reshape(79, 81, 129)
    T = np.frombuffer(blobs[1], dtype='<f8').reshape(4, 4)
    np.savez_compressed(os.path.join(OUT, 'duck-128_vox.npz'), occupancy=occ, T=T)


if __name__ == '__main__':
    main(sys.argv[1])
