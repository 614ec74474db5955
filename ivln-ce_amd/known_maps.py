"""Known-map builder: runs an iterative mapper over a stream of observations and turns the cloud each batch row explored
into a known scene - a `{scene}.npz` file of known-map mode (`mapping.save_known_scene`; what `GTSemanticsKnownMapper` /
`PredictedSemanticsKnownMapper` read from data/known_maps/{gt,predicted}_semantics) and / or an entry of a device-resident
`mapping.KnownSceneLibrary`.  The clouds leave the mapper per row and in the reference's cloud order
(include/ivln_map_build.h): the files are what the reference's iterative mapper would have written for the same frames."""
from typing import Dict, Iterable, List, Optional

import torch

from .mapping import KnownSceneLibrary, save_known_scene


def build_known_maps(batches: Iterable[dict], transformer, out_dir: Optional[str] = None,
                     library: Optional[KnownSceneLibrary] = None) -> Dict[str, int]:
    """batches: observation dicts as the `*IterativeMapper` transformers take them - depth, semantic12 (GT transformer) or
    rgb (predicted semantics), world_robot_pose, world_robot_orientation, env_name - one per step, a row per env.
    `not_done_masks` is supplied here: 0 on a row's first frame of a scene, 1 while its `env_name` stays the same, so a
    scene accumulates across episode boundaries.  When a row's scene changes (or the row leaves the batch), and at the end
    of the stream, the row's cloud is written to `{out_dir}/{scene}.npz` and / or promoted into `library`.  A scene that
    comes back after it was flushed, or that two rows are in at once, raises ValueError naming the scene: a second cloud
    never silently replaces the first.  Returns {scene: points}."""
    result: Dict[str, int] = {}
    current: List[Optional[str]] = []  # scene each row is accumulating

    def flush(b):
        scene = current[b]
        mm = transformer.mapping_module
        mm.check_status()  # a cloud that overflowed its table / capacity is not written as if it were whole
        n = None
        if out_dir is not None:
            xyz, sem = mm.export_scene(b)
            save_known_scene(out_dir, scene, xyz, sem)
            n = int(sem.shape[0])
        if library is not None:
            library.add_from_mapper(scene, mm, b)
            n = library.points(scene)
        if n is None:
            n = int(mm.env_counts()[b])
        result[scene] = n
        current[b] = None

    for batch in batches:
        names = [str(x) for x in batch["env_name"]]
        B = len(names)
        for b, scene in enumerate(current):  # before the step: it clears a row whose not_done is 0 and rows >= B
            if scene is not None and (b >= B or names[b] != scene):
                flush(b)
        del current[B:]
        current.extend([None] * (B - len(current)))
        not_done = [1 if current[b] == names[b] else 0 for b in range(B)]
        for b in range(B):
            if not_done[b] == 0:
                if names[b] in result or names[b] in current:
                    raise ValueError(f"scene {names[b]!r} appears a second time (again later, or in two rows): "
                                     "its cloud would replace the one already built")
                current[b] = names[b]
        obs = dict(batch)  # (the transformer deletes keys from the dict it is given)
        obs["not_done_masks"] = torch.tensor(not_done, dtype=torch.uint8, device=batch["depth"].device).reshape(B, 1)
        transformer(obs)
    for b, scene in enumerate(current):
        if scene is not None:
            flush(b)
    return result
