"""The host-copy rule of DESIGN.md section 3, held mechanically: in csrc/ the runtime's copy and wait calls occur only inside the
HostCopy primitives and inside the functions listed here, which are the rule's named exceptions.  No GPU, no build: it reads the sources."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "visualslam_android_amd", "csrc")

# hipMemcpy2DAsync is the enqueued form of hipMemcpy2D and falls under the same rule
CALLS = ("hipMemcpy", "hipMemcpy2D", "hipMemcpyAsync", "hipMemcpy2DAsync", "hipStreamSynchronize")
CALL_RE = re.compile(r"\b(%s)\s*\(" % "|".join(CALLS))

ALLOWED = {
    # the primitives, and the owner that waits for its streams before it gives them back
    ("vslam_internal.h", "HostCopy"),
    ("vslam_internal.h", "DevOwner"),
    # copies that are asynchronous on purpose
    ("frontend.hip", "fe_make_keyframe_lite"),      # host-frame upload, step-list staging copy
    ("reset.hip", "vslam_reset_streams"),           # pinned flag ring
    ("snapshot.hip", "vslam_snapshot_stream"),      # staged blob traffic and its closing wait
    ("snapshot.hip", "vslam_restore_stream"),
    ("ba.hip", "vslam_bundle_compute"),             # device-to-device restores
    # waits that are not about a copy
    ("system.hip", "vslam_synchronize"),
    ("ba.hip", "vslam_bundle_synchronize"),
    ("map.hip", "vslam_update"),
    ("ba.hip", "ba_sync_streams"),
    ("system.hip", "sys_acquire"),                  # the zeroing contract
    ("ba.hip", "bundle_acquire"),
    ("ba.hip", "ba_alloc"),
    ("map.hip", "vslam_profile_begin"),             # profile entry points and VSLAM_PROFILE_SERIAL
    ("map.hip", "vslam_profile_end"),
    ("map.hip", "vslam_finish_frame"),
    ("map.hip", "track_frame_rest"),
    ("ba.hip", "vslam_bundle_get_timing"),          # event-timing reads
    ("ba.hip", "vslam_get_mapmaker_timing"),
    ("reset.hip", "vslam_get_reset_timing"),
    ("snapshot.hip", "vslam_get_snapshot_timing"),
    # entry points without a handle: the null stream from start to end
    ("system.hip", "vslam_eval_transcendental"),
    ("system.hip", "vslam_eval_select"),
    ("system.hip", "vslam_eval_pose_tail"),
    ("track.hip", "vslam_pvs_permutation"),
    ("feeder_dev.hip", "vslam_feeder_render_device"),
}


def _strip(text):
    """Comments, string and character literals and preprocessor lines blanked out (newlines kept, so offsets map to lines)."""
    def blank(m):
        return re.sub(r"[^\n]", " ", m.group(0))
    text = re.sub(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])*'", blank, text, flags=re.S)
    return re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", blank, text, flags=re.M)


def _name(header):
    """The name a top-level `... {` introduces: a function's, or a struct's."""
    header = re.sub(r"__launch_bounds__\s*\([^)]*\)|__attribute__\s*\(\(.*?\)\)", " ", header)
    m = re.search(r"(\w+)\s*\(", header)
    if m:
        return m.group(1)
    m = re.search(r"\b(?:struct|class|union|enum(?:\s+class)?)\s+(\w+)", header)
    return m.group(1) if m else None


def _units(text):
    """(name, start, end) of every top-level braced unit; namespace and extern "C" blocks are looked into, not taken as units."""
    out, depth, head, i, open_at, name = [], 0, 0, 0, 0, None
    while i < len(text):
        ch = text[i]
        if ch == "{":
            if depth == 0:
                header = text[head:i]
                if re.search(r"\bnamespace\b", header) or re.fullmatch(r"\s*extern\s*", header):
                    head = i + 1            # transparent: stay at depth 0 (its closing brace is skipped below)
                    i += 1
                    continue
                name, open_at = _name(header), i
            depth += 1
        elif ch == "}":
            if depth == 0:
                head = i + 1                # end of a namespace / extern block
            else:
                depth -= 1
                if depth == 0:
                    out.append((name, open_at, i))
                    head = i + 1
        elif ch == ";" and depth == 0:
            head = i + 1
        i += 1
    assert depth == 0
    return out


def _scan():
    """{(file, unit name): [(line, call), ...]} for every call, and the set of all (file, unit name)."""
    found, units = {}, set()
    paths = sorted(p for ext in ("*.hip", "*.cpp", "*.h") for p in glob.glob(os.path.join(CSRC, ext)))
    assert len(paths) > 20, paths
    for path in paths:
        fname = os.path.basename(path)
        with open(path, encoding="utf-8") as f:
            text = _strip(f.read().replace('extern "C"', "extern    "))
        spans = _units(text)
        units.update((fname, n) for n, _, _ in spans)
        for m in CALL_RE.finditer(text):
            owner = next((n for n, a, b in spans if a < m.start() < b), None)
            found.setdefault((fname, owner), []).append((text.count("\n", 0, m.start()) + 1, m.group(1)))
    return found, units


def test_scanner_sees_the_primitives():
    found, units = _scan()
    calls = {c for _, c in found[("vslam_internal.h", "HostCopy")]}
    assert {"hipMemcpyAsync", "hipMemcpy2DAsync", "hipStreamSynchronize"} <= calls
    assert ("map.hip", "vslam_map_add_points") in units and ("boot.hip", "probe_admissible") in units


def test_runtime_copies_and_waits_only_in_primitives_and_exceptions():
    found, _ = _scan()
    stray = {k: v for k, v in found.items() if k not in ALLOWED}
    assert not stray, "copy / wait calls outside HostCopy and the exceptions of DESIGN.md section 3: %r" % stray


def test_every_exception_still_exists_and_still_needs_its_entry():
    found, units = _scan()
    for key in sorted(ALLOWED):
        assert key in units, "allow-list entry %s::%s is not a function of csrc/ any more" % key
        assert key in found, "allow-list entry %s::%s holds no copy or wait call any more: drop it" % key
