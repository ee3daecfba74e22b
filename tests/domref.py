"""populate_domain_names (src/capture.rs:1307-1411) restated in plain Python, restricted to dns_resolutions:
the reference also asks its active resolver (prioritize_resolution / add_ip_to_resolver / get_resolved_ip,
src/capture.rs:1353-1374), which is network I/O and has no counterpart here, so a side the passive
resolutions do not know stays as it is.  A restatement from the code, not output of the reference."""

EXCLUDED = ("Unknown", "Resolving")  # src/capture.rs:1381, 1389


def populate_domain_names(sessions, current, resolutions, now=None):
    """sessions: {key: {"src_ip", "dst_ip", "src_domain", "dst_domain", "last_modified"}} -- updated in place;
    current: the keys of current_sessions (the only ones walked, src/capture.rs:1322-1331); resolutions:
    {ip: name} (dns_resolutions).  Returns the keys of the sessions it modified (update_count's sessions)."""
    modified = []
    for key in current:                                           # capture.rs:1331
        info = sessions.get(key)
        if info is None:                                          # capture.rs:1378 (get_mut gave None)
            continue
        src = resolutions.get(info["src_ip"])                     # capture.rs:1346-1348
        dst = resolutions.get(info["dst_ip"])                     # capture.rs:1349-1351
        if src is None and dst is None:                           # capture.rs:1377
            continue
        mod = False
        if src is not None and src not in EXCLUDED:               # capture.rs:1380-1381
            if info.get("src_domain") != src:                     # capture.rs:1382
                info["src_domain"] = src                          # capture.rs:1383
                mod = True
        if dst is not None and dst not in EXCLUDED:               # capture.rs:1388-1389
            if info.get("dst_domain") != dst:                     # capture.rs:1390
                info["dst_domain"] = dst                          # capture.rs:1391
                mod = True
        if mod:                                                   # capture.rs:1397-1399
            info["last_modified"] = now
            modified.append(key)
    return modified


def is_current(status_byte):
    """FB_VIEW_CURRENT's predicate over a status byte: never aged since insert, or in current_sessions."""
    return status_byte == 0 or bool(status_byte & 16)
