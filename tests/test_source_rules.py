"""Rules the native sources keep that no compiler checks (CPU-only: reads the .hip files as text)."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parallelnbody_amd", "csrc")


def _functions(text):
    """(start, end) of every top-level brace block: from a line that ends with '{' at nesting depth 0 to the '}' in column 0."""
    out, start = [], None
    for m in re.finditer(r"^(.*)$", text, re.M):
        line = m.group(1)
        if start is None and line.rstrip().endswith("{") and not line.startswith((" ", "\t", "}")):
            start = m.start()
        elif start is not None and line.startswith("}"):
            out.append((start, m.end()))
            start = None
    return out


WAITS = ("hipStreamSynchronize(nullptr)", "hipDeviceSynchronize()")


def _waited(text):
    return any(w in text for w in WAITS)


def test_memsets_on_the_null_stream_are_waited_for_before_the_function_returns():
    # hipMemset returns before the fill has run, and it runs on the NULL stream; every context works on a non-blocking stream,
    # which does not wait for the null stream.  Round 4's frames fuzz found a creation memset landing inside the first frame, and
    # the fix first missed the small systems' early `return hipSuccess` in front of the wait.  So, for a function that calls
    # hipMemset(:
    #   * every `return` behind its first hipMemset( — other than the error exits that destroy the object (`return bail(`; BH_TRY's
    #     are of that kind and hidden in the macro) — has a wait for the null stream between the last hipMemset( before it and itself;
    #   * or the function waits nowhere, is `static`, and every call of it in its file is followed by the wait before the caller's
    #     next `return` (bh_create_state / bh_create).
    checked = 0
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp"))):
        text = re.sub(r"//[^\n]*", "", open(path).read())          # (comments talk about returns and memsets too)
        funcs = _functions(text)
        for a, b in funcs:
            body = text[a:b]
            first = body.find("hipMemset(")
            if first < 0:
                continue
            checked += 1
            name = os.path.basename(path) + ": " + body[:body.index("\n")]
            if not _waited(body):
                head = body[:body.index("(")]
                assert head.startswith("static "), f"{name}\ncalls hipMemset( and neither waits for the null stream nor is static"
                fn = head.split()[-1].lstrip("*")
                calls = 0
                for ca, cb in funcs:
                    caller = text[ca:cb]
                    if (ca, cb) == (a, b):
                        continue
                    for m in re.finditer(re.escape(fn) + r"\(", caller):
                        rest = caller[m.end():]
                        nxt = re.search(r"\breturn\b", rest)
                        assert nxt is not None and _waited(rest[:nxt.start()]), (
                            f"{name}\nis called without a wait for the null stream before the caller returns:\n" + caller[:200])
                        calls += 1
                assert calls >= 1, f"{name}\ncalls hipMemset(, does not wait, and no caller was found"
                continue
            for m in re.finditer(r"\breturn\b(?! bail\()", body):
                if m.start() < first:
                    continue
                last = body.rfind("hipMemset(", 0, m.start())
                assert _waited(body[last:m.start()]), (
                    f"{name}\nreturns behind a hipMemset( without waiting for the null stream:\n" + body[m.start():m.start() + 120])
    assert checked >= 2          # nbody_create and bh_create_state at least


# functions whose blocking hipMemcpy( needs no wait in front of it: by name, each with its reason
BLOCKING_COPY_EXEMPT = {
    "nbody_create": "creation: the lists of the plan and the clock word go into buffers allocated in this function, before the context's "
                    "stream has carried any work",
}
# what queues work between a wait and a copy: a kernel launch (a launcher of kernels.h, a launch written out, this library's own queue_* /
# run_* / timed_launch helpers) or any ...Async( call
QUEUES_WORK = re.compile(r"\w*Async\(|<<<|hipLaunchKernelGGL|\blaunch_\w+\(|\bqueue_\w+\(|\brun_\w+\(|\btimed_launch\(")


def blocking_copy_faults(text, where):
    """Every blocking hipMemcpy( of `text` that has no hipStreamSynchronize( earlier in its function, or has work queued between the
    last one and itself: (messages, copies looked at, names of the exempt functions in which a blocking copy was passed over)."""
    text = re.sub(r"//[^\n]*", "", text)
    faults, checked, exempt_used = [], 0, set()
    for a, b in _functions(text):
        body = text[a:b]
        head = body[:body.index("(")] if "(" in body else body
        fn = head.split()[-1].lstrip("*&") if head.split() else ""
        for m in re.finditer(r"\bhipMemcpy\(", body):
            if fn in BLOCKING_COPY_EXEMPT:
                exempt_used.add(fn)
                continue
            checked += 1
            line = body[:m.start()].count("\n")
            # the last wait whose block is still open at the copy: one in a branch that has closed since (an `if` arm beside the
            # copy's own) is not on the copy's path
            wait = body.rfind("hipStreamSynchronize(", 0, m.start())
            while wait >= 0:
                depth, low = 0, 0
                for ch in body[wait:m.start()]:
                    depth += (ch == "{") - (ch == "}")
                    low = min(low, depth)
                if low == 0:
                    break
                wait = body.rfind("hipStreamSynchronize(", 0, wait)
            if wait < 0:
                faults.append(f"{where}: {fn}: blocking hipMemcpy( (line {line} of the function) with no hipStreamSynchronize( before it in "
                              "the function: it runs on the null stream, which the context's non-blocking stream does not wait for")
                continue
            between = QUEUES_WORK.search(body, wait + len("hipStreamSynchronize("), m.start())
            if between:
                faults.append(f"{where}: {fn}: '{between.group(0)}' queues work between the last hipStreamSynchronize( and the blocking "
                              f"hipMemcpy( (line {line} of the function)")
    return faults, checked, exempt_used


def test_blocking_copies_wait_for_the_stream_first():
    # hipMemcpy( runs on the NULL stream and the contexts' streams are non-blocking: a copy into or out of a buffer that queued work
    # still writes races with it unless the function has waited for the stream and queued nothing since.  upload_soa's converting
    # branches did not (an fp64 context given floats, an fp32 one given doubles): steps in flight wrote their update on top of the
    # uploaded state.  The rule is per function: a wait somewhere up the call chain does not count (set_particles relied on
    # upload_soa's).
    faults, checked, exempt_used = [], 0, set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp"))):
        f, k, used = blocking_copy_faults(open(path).read(), os.path.basename(path))
        faults += f
        checked += k
        exempt_used |= used
    assert not faults, "\n".join(faults)
    assert checked >= 10, checked      # (the rule cannot pass on nothing)
    # every exemption is still needed: a function of that name, in a .hip or .cpp file, with a blocking copy the rule passed over
    assert exempt_used == set(BLOCKING_COPY_EXEMPT), sorted(set(BLOCKING_COPY_EXEMPT) - exempt_used)


def test_no_stream_is_created_blocking_by_accident():
    # (the rule above rests on it: the streams are non-blocking on purpose — a blocking stream would serialise with torch's
    # null-stream work in the host process)
    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        text = open(path).read()
        assert "hipStreamCreate(" not in text, path
