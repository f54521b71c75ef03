"""Image -> supervoxel graph (the reference's mri2graph package), on the MI355X."""
