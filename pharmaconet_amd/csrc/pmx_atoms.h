// pmx_atoms.h - what stands behind the opaque pmx_atoms of include/pmx.h (host only): the device copy of an atom store, for the units that
// take such a handle. pmx_atoms.hip makes, reads and destroys it; pmx_pose_search.hip reads its device and its largest record.
#pragma once
#include <cstdint>

#include "pmx.h"

struct pmx_atoms {
    int device = 0;
    uint64_t *offsets = nullptr; // [n_ligands + 1]
    uint8_t *data = nullptr;     // the records, validated by pmx_atoms_upload: a kernel may trust every header and every element
    float *radius = nullptr;     // [128] by atomic number
    pmx_atoms_info info{};
};
