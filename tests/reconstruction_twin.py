"""The reconstruction chain on the host with the C++ twins in place of the numpy restatements: the backend that
reconstruction_cases.run_chain composes into the host chain the device chain is held to, word for word.

There is no arithmetic here.  Every stage goes through its twin's existing driver (fundamental_twin.verify, pose_twin.run,
triangulate_twin.run, resect_twin.run, bundle_twin.run, bundle_intr_twin.run) and takes the previous stage's output words; the
tables between them are reconstruction_cases' integer-exact numpy restatements."""
import numpy as np

import bundle_intr_twin
import bundle_twin
import fundamental_twin
import pose_twin
import reconstruction_cases as cases
import resect_twin
import triangulate_twin

FILL = bundle_twin.FILL
assert FILL == pose_twin.FILL == triangulate_twin.FILL == resect_twin.FILL == bundle_intr_twin.FILL


class Twins:
    """the five programs, compiled once into `tmp`, as a backend of reconstruction_cases.run_chain"""

    def __init__(self, tmp):
        self.tmp = tmp
        self.exe = {m.__name__: m.build(tmp) for m in (fundamental_twin, pose_twin, triangulate_twin, resect_twin, bundle_twin,
                                                      bundle_intr_twin)}
        self._verified = {}

    def verify(self, e, ka, kb, match, n_hyp, thr, seed):
        # (F does not depend on the intrinsics: the two scenes of one collection share it)
        key = (ka.tobytes(), kb.tobytes(), match.tobytes(), n_hyp, thr, seed)
        if key not in self._verified:
            r = fundamental_twin.verify(self.exe["fundamental_twin"], self.tmp, ka, kb, match, n_hyp, thr, seed)
            self._verified[key] = (r["F"].reshape(9), r["verified"], r["stats"])
        return self._verified[key]

    def pose(self, table, deg):
        return pose_twin.run(self.exe["pose_twin"], self.tmp, table, deg)

    def triangulate(self, table, px, rounds):
        r = triangulate_twin.run(self.exe["triangulate_twin"], self.tmp, table, px, rounds)
        return dict(r, obs_state=r["obs_state"][:int(table["counts"][1])])

    def resect(self, sc, **kw):
        return resect_twin.run(self.exe["resect_twin"], self.tmp, sc, **kw)

    def bundle(self, sc, **kw):
        return bundle_twin.run(self.exe["bundle_twin"], self.tmp, sc, **kw)

    def bundle_intrinsics(self, sc, refine, **kw):
        return bundle_intr_twin.run(self.exe["bundle_intr_twin"], self.tmp, sc, refine=refine, **kw)


def run(twins, scene, K, focal=False, params=cases.PARAMS):
    """the host chain: every stage's output words, the resection and triangulation once per round"""
    return cases.run_chain(scene, K, twins, focal=focal, params=params)
