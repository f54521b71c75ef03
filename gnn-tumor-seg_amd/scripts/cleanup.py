"""The connected-component clean-up flags of the prediction CLIs (segment_scans, generate_gnn_predictions,
generate_joint_predictions), defined once.  With every flag at its default `from_args` returns None and
gts.components is never imported: the CLIs then write what they always wrote."""

BRATS_ET_LABEL = 4           # enhancing tumour in BraTS coding, and what a too-small total of it becomes:
BRATS_ET_REPLACEMENT = 1     # necrotic core

# (name, type, default, choices, help)
FLAGS = (
    ("--min_component_voxels", int, 0, None,
     "drop connected components of the predicted whole tumour with fewer voxels than this (0: off)"),
    ("--connectivity", int, 26, (6, 26), "voxel neighbourhood of a component: 6 (faces) or 26 (faces, edges, corners)"),
    ("--min_enhancing_voxels", int, 0, None,
     "relabel the enhancing tumour to necrotic core when fewer voxels of it than this remain (0: off)"),
)
STAT_NAMES = ("components", "components_removed", "voxels_removed", "et_relabelled")


def add_flags(parser):
    for name, kind, default, choices, text in FLAGS:
        parser.add_argument(name, type=kind, default=default, choices=choices, help=text)
    return parser


class Cleanup:
    """The clean-up a command line asked for; called on a device label volume in BraTS coding."""

    def __init__(self, min_component_voxels=0, connectivity=26, min_enhancing_voxels=0):
        self.min_voxels = int(min_component_voxels)
        self.connectivity = int(connectivity)
        self.et_min_voxels = int(min_enhancing_voxels)
        self.last_stats = None      # device int64 [4] of the latest __call__, for the scan's line of output

    @property
    def drops_components(self):
        return self.min_voxels > 0

    def __call__(self, labels):
        """Filtered int16 device volume (gts.components.remove_small_components, both rules)."""
        from gts import components

        out, self.last_stats = components.remove_small_components(
            labels, self.min_voxels, self.connectivity, et_label=BRATS_ET_LABEL, et_min_voxels=self.et_min_voxels,
            et_replacement=BRATS_ET_REPLACEMENT)
        return out

    def surviving(self, labels):
        """labels without its small components: the component rule alone, for the CNN's crop box."""
        from gts import components

        return components.remove_small_components(labels, self.min_voxels, self.connectivity)[0]

    def report(self):
        """'components 3, components_removed 1, ...' of the latest __call__ (one small copy)."""
        return ", ".join(f"{name} {value}" for name, value in zip(STAT_NAMES, self.last_stats.cpu().tolist()))


def from_args(args):
    """The Cleanup of parsed arguments, or None when every flag is at its default."""
    picked = Cleanup(args.min_component_voxels, args.connectivity, args.min_enhancing_voxels)
    return picked if picked.min_voxels > 0 or picked.et_min_voxels > 0 else None
