"""Mirror of the reference's detector3d/tools package, as far as it is device work: train_utils.optimization."""
