/*
 * ORACLE -- TEST INFRASTRUCTURE ONLY.  Included by mapper_oracle.c (it uses that file's SiteScore / GapTools / list helpers).
 *
 * The FINAL ALIGNMENT STAGE: everything BBMapThread.processRead / processReadPair do after the rescue stage, i.e. the calls that
 * produce the coordinates, the score and the match string (CIGAR) BBMap prints (paths relative to /root/reference):
 *   processRead tail        current/align2/BBMapThread.java:492-732   (setPerfectFlag, clearzone / ambiguity, low-quality removal,
 *                                                                     the genMatchString loop, removeDuplicateBestSites, applyClearzone3,
 *                                                                     toLocalAlignment for clipped strings, tip penalty)
 *   processReadPair tail    current/align2/BBMapThread.java:1116-1356 (removeLowQualitySitesPaired, pairSiteScoresFinal, ambiguity,
 *                                                                     canPair, genMatchString per mate, toLocalAlignment)
 *   genMatchString          current/align2/AbstractMapThread.java:860-965
 *   genMatchStringForSite   current/align2/AbstractMapThread.java:968-1068
 *   realign_new             current/align2/TranslateColorspaceRead.java:229-653 (<= 3 fillLimited + 1 fillUnlimited, score, traceback)
 *   SiteScore               current/stream/SiteScore.java:430-491 (matchContainsXY, left/rightPaddingNeeded), :493-681 (clipTipIndels,
 *                           clipLeft/RightTipIndel, unclip), :686-838 fixXY, :916-931 fixLimitsXY, :227-233 setPerfectFlag
 *   MSA                     current/align2/MSA.java:216-484 toLocalAlignment, :488-558 score(match), :726-747 calcMatch/Sub/Noref/NocallScore
 *   Read                    current/stream/Read.java:1172-1190 setFromSite, :1202-1262 setFromTopSite, :1269-1286 clearMapping / clearSite,
 *                           :1419-1469 calcMatchLength, :2051-2056 containsXYC, :2494-2512 setPerfectFlag, :3141-3150 CHECKORDER
 *   AbstractMapThread       :1328-1349 removeDuplicateBestSites, :1820-1910 applyClearzone3, :1919-2095 pairSiteScoresFinal,
 *                           :2097-2164 canPair, :2499-2609 calcTipScorePenalty / applyScorePenalty
 *   Tools                   current/align2/Tools.java:913-930 countTopScores, :986-1003 removeLowQualitySitesUnpaired
 * Configuration: bbmap.sh defaults -- ambiguous=best (AMBIGUOUS_TOSS = AMBIGUOUS_RANDOM = false), KILL_BAD_PAIRS = false,
 * LOCAL_ALIGN = false, PRINT_SECONDARY_ALIGNMENTS = false, STRICT_MAX_INDEL = false, no identity / edit filters (postFilterRead and
 * ensureMatchStringOnPrimary then change nothing), USE_SS_MATCH_FOR_PRIMARY = GEN_MATCH_FAST = true (AbstractMapThread.java:2850, :2929).
 * NOT restated: DYNAMIC_INSERT_LENGTH's running average (BBMapThread.java:1307-1309; the caller feeds averagePairDist), statistics.
 * PARITY STATUS: restatement only (Java; no JVM here); pinned through tests/test_golden_phix.py (the reference's PhiX fixture, whose
 * read names hold the true coordinates this stage is graded against by AbstractMapThread.isCorrectHit).
 */

/* branch counters for the tests (which of the rare paths a test really took; not thread-safe: meaningful after single-threaded runs):
 * [0] clipTipIndels clipped, [1] fixXY on a string with X / Y, [2] toLocalAlignment called, [3] ... and it clipped, [4] realign_new's
 * tail recursion, [5] genMatchStringForSite's second realign_new, [6] genMatchString's re-sort loop, [7] processRead's do-while repeated,
 * [8] a site beyond the first got a match string, [9] removeDuplicateBestSites removed one */
static int64_t g_branch[16];
void orc_final_branch_counts(int64_t *out16, int reset) { memcpy(out16, g_branch, sizeof g_branch); if (reset) memset(g_branch, 0, sizeof g_branch); }

/* ------------------------------------------------------------------ match strings: a per-pair arena, sites carry ids */
#define SITE_MATCH(ss) ((ss)->reserved[0])        /* arena id, 0 = match == null */
#define SITE_OBJ(ss) ((ss)->reserved[1])          /* object identity (Java compares SiteScore references, AbstractMapThread.java:939) */

static int m_new(mapper *M, int len) {
    if (M->nms == M->mscap) { M->mscap = M->mscap ? 2 * M->mscap : 64; M->ms = (mstr *)realloc(M->ms, sizeof(mstr) * (size_t)M->mscap); }
    M->ms[M->nms].p = (uint8_t *)malloc((size_t)len + 1); M->ms[M->nms].len = len;
    return ++M->nms;
}
static void m_reset(mapper *M) { for (int i = 0; i < M->nms; i++) free(M->ms[i].p); M->nms = 0; }
static inline mstr *m_get(mapper *M, int id) { return id > 0 ? &M->ms[id - 1] : NULL; }

typedef struct {                   /* stream.Read's mapping state */
    int mapped, paired, ambiguous, perfect, rescued;
    int chrom, strand, start, stop, mapScore;
    int ngaps; int32_t gaps[ORC_MAX_GAPS];
    int match;                     /* arena id (Read.match aliases a SiteScore's array), 0 = null */
    int L; const uint8_t *bp, *bm; /* bases, reverse complement */
    int64_t numericID;
} rstate;

static uint8_t ca_get(const orc_index *ix, int chrom, int loc) {            /* ChromosomeArray.get (current/dna/ChromosomeArray.java:232-234) */
    const int maxIndex = ix->chromArrLen[chrom] - 1;
    return (loc < 0 || loc >= maxIndex) ? (uint8_t)'N' : ix->chromArr[chrom][loc];
}
static int fully_defined_b(uint8_t b) { return b < 128 && orc_base_to_number()[b] >= 0; }   /* AminoAcid.isFullyDefined(byte) :365-367 */

/* Read.calcMatchLength (Read.java:1419-1469) */
static int calc_match_length(const uint8_t *match, int n) {
    if (!match || n < 1) return 0;
    uint8_t mode = '0', c = '0'; int current = 0, len = 0;
    for (int i = 0; i < n; i++) {
        c = match[i];
        if (c >= '0' && c <= '9') current = current * 10 + (c - '0');
        else if (mode == c) current = imax(current + 1, 2);
        else {
            current = imax(current, 1);
            if (mode == 'm' || mode == 'S' || mode == 'D' || mode == 'C' || mode == 'X' || mode == 'Y' || mode == 'N' || mode == 'R') len += current;
            mode = c; current = 0;
        }
    }
    if (current > 0 || !(c >= '0' && c <= '9')) {
        current = imax(current, 1);
        if (mode == 'm' || mode == 'S' || mode == 'D' || mode == 'C' || mode == 'X' || mode == 'Y' || mode == 'N' || mode == 'R') len += current;
    }
    return len;
}
static int lengths_agree(mapper *M, const orc_msite *ss) {                  /* SiteScore.java:840-851 */
    const mstr *m = m_get(M, SITE_MATCH(ss));
    return !m ? 1 : calc_match_length(m->p, m->len) == ss->stop - ss->start + 1;
}
static int match_contains_xy(mapper *M, const orc_msite *ss) {              /* :430-434 */
    const mstr *m = m_get(M, SITE_MATCH(ss));
    if (!m || m->len < 1) return 0;
    const uint8_t a = m->p[0], b = m->p[m->len - 1];
    return a == 'X' || a == 'Y' || b == 'X' || b == 'Y';
}

/* MSA.calcSubScore / calcMatchScore (MSA.java:726-747), MSA.score(match) (:488-558) */
#ifdef ORC_PACBIO
enum { F_MATCH = 90, F_MATCH2 = 100, F_SUB = -137, F_SUBR = -157, F_SUB2 = -49, F_SUB3 = -25, F_LIM3 = 5 };
#else
enum { F_MATCH = 70, F_MATCH2 = 100, F_SUB = -127, F_SUBR = -147, F_SUB2 = -51, F_SUB3 = -25, F_LIM3 = 5 };
#endif
static int calc_sub_score(int len) {
    int score = F_SUB;
    if (len > F_LIM3) { score += (len - F_LIM3) * F_SUB3; len = F_LIM3; }
    if (len > 1) score += (len - 1) * F_SUB2;
    return score;
}
static int msa_score_mode(uint8_t mode, int current, uint8_t prevMode, int prevStreak) {
    if (mode == 'm') return F_MATCH + (current - 1) * F_MATCH2;
    if (mode == 'S') {
        int s = calc_sub_score(current);
        if (prevMode == 'N' || prevMode == 'R') s += F_SUB2 - F_SUB;
        else if (prevMode == 'm' && prevStreak < 2) s += F_SUBR - F_SUB;
        return s;
    }
    if (mode == 'D') return orc_calc_del_score(current, 1);
    if (mode == 'I' || mode == 'X' || mode == 'Y') return orc_calc_ins_score(current);
    return 0;                      /* 'C': nothing; 'N' / 'R': POINTS_NOCALL = POINTS_NOREF = 0 */
}
static int msa_score_match(const uint8_t *match, int n) {
    if (!match || n < 1) return 0;
    uint8_t mode = match[0], prevMode = '0'; int current = 0, prevStreak = 0, score = 0;
    for (int mpos = 0; mpos < n; mpos++) {
        const uint8_t c = match[mpos];
        if (mode == c) current++;
        else { score += msa_score_mode(mode, current, prevMode, prevStreak); prevMode = mode; prevStreak = current; mode = c; current = 1; }
    }
    if (current > 0) score += msa_score_mode(mode, current, prevMode, prevStreak);
    return score;
}

/* SiteScore.leftPaddingNeeded / rightPaddingNeeded (:448-491), literally (the right-hand loop tests mloc >= tiplen as the left one does) */
static int left_padding_needed(mapper *M, const orc_msite *ss, int tiplen, int maxIndel) {
    const mstr *m = m_get(M, SITE_MATCH(ss));
    if (!m || m->len < 1) return 0;
    int insertion = 0, xy = 0;
    for (int mloc = 0; mloc < m->len; mloc++) {
        const uint8_t c = m->p[mloc];
        if (c == 'I') insertion++;
        else if (c == 'X' || c == 'Y') xy++;
        else if (c == 'D') return insertion + xy;
        else if (mloc >= tiplen) break;
    }
    if (insertion > maxIndel || xy > 0 || m->p[0] == 'I') return insertion + xy;
    return 0;
}
static int right_padding_needed(mapper *M, const orc_msite *ss, int tiplen, int maxIndel) {
    const mstr *m = m_get(M, SITE_MATCH(ss));
    if (!m || m->len < 1) return 0;
    const int lastIndex = m->len - 1;
    int insertion = 0, xy = 0;
    for (int mloc = lastIndex; mloc >= 0; mloc--) {
        const uint8_t c = m->p[mloc];
        if (c == 'I') insertion++;
        else if (c == 'X' || c == 'Y') xy++;
        else if (c == 'D') return insertion + xy;
        else if (mloc >= tiplen) break;
    }
    if (insertion > maxIndel || xy > 0 || m->p[lastIndex] == 'I') return insertion + xy;
    return 0;
}

/* SiteScore.clipLeftTipIndel (:523-575) */
static int clip_left_tip_indel(mapper *M, orc_msite *ss, int tiplen, int maxIndel) {
    mstr *m = m_get(M, SITE_MATCH(ss));
    if (!m || m->len < maxIndel) return 0;
    uint8_t *match = m->p; const int n = m->len;
    if (match[0] == 'C' || match[0] == 'Y' || match[0] == 'X') return 0;
    int neutral = 0, insertion = 0, deletion = 0;
    {
        int mloc = 0;
        for (; mloc < n; mloc++) {
            const uint8_t c = match[mloc];
            if (c == 'I') insertion++;
            else if (c == 'D') deletion++;
            else { neutral++; if (mloc >= tiplen) break; }
        }
        /* `while(mloc>=0 && match[mloc]=='m')`: when the scan ran off the end, Java's match[mloc] throws; such strings (nothing but a short
         * tip) do not reach this function with match.length >= maxIndel (10) and tiplen 4 */
        while (mloc >= 0 && mloc < n && match[mloc] == 'm') { mloc--; neutral--; }
    }
    if (insertion <= maxIndel && deletion <= 4 * maxIndel) return 0;
    int sum = neutral + insertion + deletion;
    if (deletion > 0) {
        const int id = m_new(M, n - deletion);
        m = m_get(M, SITE_MATCH(ss));                     /* the arena may have moved */
        match = m->p;
        uint8_t *temp = M->ms[id - 1].p;
        int i = 0, j = 0;
        for (; i < sum; i++) if (match[i] != 'D') temp[j++] = match[i];
        for (; i < n; i++, j++) temp[j] = match[i];
        SITE_MATCH(ss) = id;
        match = temp;
    }
    sum = neutral + insertion;
    for (int i = 0; i < sum; i++) match[i] = 'C';
    set_start(ss, ss->start - (insertion - deletion));    /* incrementStart(-dif) */
    return 1;
}
/* SiteScore.clipRightTipIndel (:577-636) */
static int clip_right_tip_indel(mapper *M, orc_msite *ss, int tiplen, int maxIndel) {
    mstr *m = m_get(M, SITE_MATCH(ss));
    if (!m || m->len < maxIndel) return 0;
    uint8_t *match = m->p; int n = m->len;
    const int lastIndex = n - 1;
    if (match[lastIndex] == 'C' || match[lastIndex] == 'Y' || match[lastIndex] == 'X') return 0;
    int neutral = 0, insertion = 0, deletion = 0;
    {
        int mloc = lastIndex;
        for (const int min = lastIndex - tiplen; mloc >= 0; mloc--) {
            const uint8_t c = match[mloc];
            if (c == 'I') insertion++;
            else if (c == 'D') deletion++;
            else { neutral++; if (mloc <= min) break; }
        }
        while (mloc >= 0 && mloc < n && match[mloc] == 'm') { mloc++; neutral--; }
    }
    if (insertion <= maxIndel && deletion <= 4 * maxIndel) return 0;
    int sum = neutral + insertion + deletion;
    const int limit = n - sum;
    if (deletion > 0) {
        const int id = m_new(M, n - deletion);
        m = m_get(M, SITE_MATCH(ss));
        match = m->p;
        uint8_t *temp = M->ms[id - 1].p;
        int i = 0, j = 0;
        for (; i < limit; i++, j++) temp[j] = match[i];
        for (; i < n; i++) if (match[i] != 'D') temp[j++] = match[i];
        SITE_MATCH(ss) = id;
        match = temp; n = n - deletion;
    }
    for (int i = limit; i < n; i++) match[i] = 'C';
    set_stop(ss, ss->stop + (insertion - deletion));      /* incrementStop(dif) */
    return 1;
}
/* SiteScore.unclip (:638-681) */
static void unclip(mapper *M, orc_msite *ss, const uint8_t *bases) {
    mstr *m = m_get(M, SITE_MATCH(ss));
    if (!m || m->len < 1) return;
    if (m->p[0] != 'C' && m->p[m->len - 1] != 'C') return;
    for (int rloc = ss->start, cloc = 0, mloc = 0; mloc < m->len; mloc++) {
        const uint8_t mm = m->p[mloc];
        if (mm == 'C') {
            const uint8_t c = bases[cloc], r = ca_get(M->ix, ss->chrom, rloc);
            if (!fully_defined_b(c) || !fully_defined_b(r)) m->p[mloc] = 'N';
            else m->p[mloc] = (c == r ? 'm' : 'S');
            rloc++; cloc++;
        } else if (mm == 'm' || mm == 'N' || mm == 'S' || mm == 'X' || mm == 'Y') { rloc++; cloc++; }
        else if (mm == 'I') cloc++;
        else if (mm == 'D') rloc++;
    }
}
/* SiteScore.clipTipIndels(bases, tiplen, maxIndel, msa) (:497-521) */
static int clip_tip_indels(mapper *M, orc_msite *ss, const uint8_t *bases, int L, int tiplen, int maxIndel) {
    const mstr *m = m_get(M, SITE_MATCH(ss));
    if (!m || m->len < maxIndel) return 0;
    const int left = clip_left_tip_indel(M, ss, tiplen, maxIndel);
    const int right = clip_right_tip_indel(M, ss, tiplen, maxIndel);
    if (left || right) {
        g_branch[0]++;
        unclip(M, ss, bases);
        const int oldScore = ss->slowScore;
        m = m_get(M, SITE_MATCH(ss));
        set_slow_score(ss, msa_score_match(m->p, m->len));
        ss->score = ss->score + (ss->slowScore - oldScore);
        site_set_perfect(ss, bases, L, M->ix);
    }
    return left | right;
}

/* SiteScore.fixXY(bases, nullifyOnFailure = false, msa) (:686-838) */
static int fix_xy(mapper *M, orc_msite *ss, const uint8_t *bases, int L) {
    if (!match_contains_xy(M, ss)) return 1;
    g_branch[1]++;
    mstr *m = m_get(M, SITE_MATCH(ss));
    uint8_t *match = m->p; const int n = m->len;
    int success = 1;
    const float maxSubRate = 0.4f; const int maxSubs = 5;
    {   /* left side */
        int mloc = 0;
        while (mloc < n && (match[mloc] == 'X' || match[mloc] == 'Y')) mloc++;
        if (mloc >= n || mloc >= L) success = 0;
        else if (mloc > 0) {
            mloc--;
            const int numX = mloc + 1;
            int rloc = ss->start + mloc, cloc = mloc, subs = 0, firstSub = -1;
            while (mloc >= 0) {
                const uint8_t c = bases[cloc], r = ca_get(M->ix, ss->chrom, rloc);
                if (r == 'N' || c == 'N') match[mloc] = 'N';
                else if (c == r) match[mloc] = 'm';
                else { match[mloc] = 'S'; subs++; if (subs == 1) firstSub = mloc; }
                mloc--; rloc--; cloc--;
            }
            if (success && (ss->stop - ss->start + 1) != calc_match_length(match, n)) set_start(ss, ss->start - numX);
            if (subs > maxSubs && (float)subs > (float)numX * maxSubRate) {
                for (int i = 0; i <= firstSub; i++) match[i] = 'C';
                /* `if(!lengthsAgree()){assert(false); ...}`: with -ea the reference stops here; clipping with 'C' keeps the length */
            }
        }
    }
    if (success) {   /* right side */
        int mloc = n - 1;
        while (mloc >= 0 && (match[mloc] == 'X' || match[mloc] == 'Y')) mloc--;
        const int dif = n - 1 - mloc;
        if (mloc < 0) success = 0;
        else if (dif > 0) {
            mloc++;
            const int numX = n - mloc;
            int rloc = ss->stop - dif + 1, cloc = L - dif, subs = 0, firstSub = -1;
            if (cloc < 0) success = 0;
            else {
                while (mloc < n) {
                    const uint8_t c = bases[cloc], r = ca_get(M->ix, ss->chrom, rloc);
                    if (r == 'N' || c == 'N') match[mloc] = 'N';
                    else if (c == r) match[mloc] = 'm';
                    else { match[mloc] = 'S'; subs++; if (subs == 1) firstSub = mloc; }
                    mloc++; rloc++; cloc++;
                }
            }
            if (success) {
                if ((ss->stop - ss->start + 1) != calc_match_length(match, n)) set_stop(ss, ss->stop + numX);
                if (subs > maxSubs && (float)subs > (float)numX * maxSubRate) for (int i = firstSub; i < n; i++) match[i] = 'C';
            }
        }
    }
    success = success && !match_contains_xy(M, ss);
    {   /* match != null (nullifyOnFailure is false at every call site of this flow) */
        const int oldScore = ss->slowScore;
        set_slow_score(ss, msa_score_match(match, n));
        ss->score = ss->score + (ss->slowScore - oldScore);
    }
    site_set_perfect(ss, bases, L, M->ix);
    return success;
}
/* SiteScore.fixLimitsXY (:916-931) */
static void fix_limits_xy(mapper *M, orc_msite *ss) {
    const mstr *m = m_get(M, SITE_MATCH(ss));
    if (!m || m->len < 1) return;
    int y = 0;
    for (int i = m->len - 1; i >= 0; i--) { if (m->p[i] == 'Y') y++; else break; }
    if (y != 0) set_limits(ss, ss->start, ss->stop + y);
}

/* ------------------------------------------------------------------ realign_new (TranslateColorspaceRead.java:229-653) */
/* one MSA fill of the final stage: fillLimited / fillUnlimited + score, logged like scoreSlow's fills.  kind: 3 first fill, 4 padded
 * refill, 5 third fill, 6 fillUnlimited.  Returns score's length (0 = max == null); mx = {rows, maxCol, maxState, maxScore}. */
static int final_fill(mapper *M, int which, int kind, const uint8_t *bases, int L, const orc_msite *ss, int minLoc, int maxLoc,
                      int minscore, int32_t *sc, int32_t *mx, int *jobOut) {
    const uint8_t *c = M->ix->chromArr[ss->chrom]; const int cl = M->ix->chromArrLen[ss->chrom];
    const int64_t it0 = M->msa->iterationsLimited + M->msa->iterationsUnlimited;
    int gcopy[ORC_MAX_GAPS]; memcpy(gcopy, ss->gaps, sizeof gcopy);
    int ok;
    if (kind == 6) ok = orc_fill_unlimited(M->msa, bases, L, c, cl, minLoc, maxLoc, ss->ngaps ? gcopy : NULL, ss->ngaps, mx);
    else ok = orc_fill_limited(M->msa, bases, L, c, cl, minLoc, maxLoc, minscore, ss->ngaps ? gcopy : NULL, ss->ngaps, mx);
    const int n = ok ? orc_score(M->msa, bases, c, minLoc, maxLoc, mx[0], mx[1], mx[2], ss->ngaps ? 1 : 0, sc) : 0;
    const int64_t it = M->msa->iterationsLimited + M->msa->iterationsUnlimited - it0;
    M->dpJobs++; M->cells += it; M->finalFills++;
    *jobOut = -1;
    if (M->log) {
        const int64_t k = __sync_fetch_and_add(M->nlog, 1);
        if (k < M->logcap) {
            *jobOut = (int)k;
            orc_mjob *j = &M->log[k]; memset(j, 0, sizeof *j);
            j->read = (int32_t)M->readIdx[which]; j->seq = M->seq[which]; j->kind = kind; j->strand = ss->strand; j->chrom = ss->chrom;
            j->refStartLoc = minLoc; j->refEndLoc = maxLoc; j->minScore = minscore; j->ngaps = ss->ngaps;
            j->score_len = n; for (int i = 0; i < n; i++) j->score[i] = sc[i];
            j->iterations = it; j->match_len = 0;
            if (n) {           /* the traceback of THIS fill, as scoreSlow's log entries carry it (realign_new itself only traces its last fill) */
                int mlen = orc_traceback(M->msa, bases, c, minLoc, maxLoc, mx[0], mx[1], mx[2], ss->ngaps ? 1 : 0, M->tb, M->tbcap);
                if (mlen < 0) mlen = 0;
                j->match_len = mlen;
                if (M->match && mlen > 0 && mlen <= M->matchStride) memcpy(M->match + k * (int64_t)M->matchStride, M->tb, (size_t)mlen);
            }
        }
    }
    M->seq[which]++;
    return n;
}

/* the padding adjustment that appears five times in realign_new (:380-405 and its copies); fixed = the minus-strand first copy (:534-555),
 * which lacks the else-branch when there is no gap array */
static void adjust_extra_pad(const orc_msa *msa, int L, const orc_msite *ss, int minLoc, int maxLoc, int *extraPadLeft, int *extraPadRight, int noFloorWhenUngapped) {
    const int maxColumns = msa->maxColumns;
    int newlen;
    if (ss->ngaps == 0) newlen = (maxLoc - minLoc + 1 + *extraPadLeft + *extraPadRight);
    else {
        orc_msite t = *ss; t.start = minLoc; t.stop = maxLoc;                     /* GapTools.calcGrefLen(minLoc, maxLoc, ss.gaps) */
        newlen = (imax(L, calc_gref_len(&t)) + 1 + *extraPadLeft + *extraPadRight);
    }
    if (newlen >= maxColumns - 80) {
        while (newlen >= maxColumns - 80 && *extraPadLeft > *extraPadRight) { newlen--; (*extraPadLeft)--; }
        while (newlen >= maxColumns - 80 && *extraPadLeft < *extraPadRight) { newlen--; (*extraPadRight)--; }
        while (newlen >= maxColumns - 80) { newlen -= 2; (*extraPadLeft)--; (*extraPadRight)--; }
    } else if (!(noFloorWhenUngapped && ss->ngaps == 0)) {
        const int x = imax(0, imin(20, ((maxColumns - newlen) / 2) - 40));
        *extraPadLeft = imax(x, *extraPadLeft); *extraPadRight = imax(x, *extraPadRight);
    }
}

static void realign_new(mapper *M, int which, orc_msite *ss, const uint8_t *bases, int L, int padding, int recur, int minValidScore,
                        int forbidIndels, int fixXY) {
    orc_msa *msa = M->msa;
    if (match_contains_xy(M, ss)) fix_xy(M, ss, bases, L);
    clip_tip_indels(M, ss, bases, L, 4, 10);
    padding = imin(padding, (msa->maxColumns - L) / 2 - 20);
    padding = imax(padding, 0);
    const uint8_t *ref = M->ix->chromArr[ss->chrom]; const int reflen = M->ix->chromArrLen[ss->chrom];
    const int maxIndex = reflen - 1;
    {
        const int expectedLen = calc_gref_len(ss);
        if (expectedLen > msa->maxColumns - 20) {
            set_stop(ss, ss->start + imin(L + 40, msa->maxColumns - 20));
            if (ss->ngaps) fix_gaps(ss, ss->start, ss->stop);
        }
    }
    if (ss->start < 0) set_start(ss, 0);
    if (ss->stop > maxIndex) set_stop(ss, maxIndex);
    {
        const int a = L, b = ss->stop - ss->start + 1;
        if (b < a) { const int c = imin(L, a - b + 10) / 2; padding = imax(padding, c + 1); }
    }
    padding = imax(0, imin(padding, (msa->maxColumns - imax(L, calc_gref_len(ss))) / 2 - 100));
    if (forbidIndels) padding = 0;
    const int maxI = orc_max_imperfect_score(L);

    /* the match array is reused when it already has the read's length, else a new one of that length (:317-325, :489-497) */
    {
        const mstr *m = m_get(M, SITE_MATCH(ss));
        if (!(m && m->len == L)) SITE_MATCH(ss) = m_new(M, L);
    }
    const int scoreNoIndel = orc_score_no_indels_match(bases, L, ref, reflen, NULL, ss->start, m_get(M, SITE_MATCH(ss))->p);
    if (scoreNoIndel >= maxI || forbidIndels) {
        set_stop(ss, ss->start + L - 1);
        set_slow_score(ss, scoreNoIndel);
    } else {
        int minLoc = imax(ss->start - padding, 0), maxLoc = imin(ss->stop + padding, maxIndex);
        int32_t sc[8], mx[4]; int n, haveMax, job = -1;
        const int minscore = imax(scoreNoIndel, minValidScore);
        n = final_fill(M, which, 3, bases, L, ss, minLoc, maxLoc, minscore, sc, mx, &job); haveMax = n > 0;
        if (n > 6) {
            int32_t old0 = sc[0];
            int extraPadLeft = sc[6], extraPadRight = sc[7];
            adjust_extra_pad(msa, L, ss, minLoc, maxLoc, &extraPadLeft, &extraPadRight, ss->strand != 0);
            minLoc = imax(0, minLoc - extraPadLeft); maxLoc = imin(maxIndex, maxLoc + extraPadRight);
            n = final_fill(M, which, 4, bases, L, ss, minLoc, maxLoc, minscore, sc, mx, &job); haveMax = n > 0;
            if (n == 0 || sc[0] < old0) {
                adjust_extra_pad(msa, L, ss, minLoc, maxLoc, &extraPadLeft, &extraPadRight, 0);
                minLoc = imax(0, minLoc - extraPadLeft); maxLoc = imin(maxIndex, maxLoc + extraPadRight);
                n = final_fill(M, which, 5, bases, L, ss, minLoc, maxLoc, minscore, sc, mx, &job); haveMax = n > 0;
                if (ss->strand == 0 && minLoc > 0 && maxLoc < maxIndex && (n == 0 || sc[0] < old0)) {           /* plus strand only (:453-459) */
                    minLoc = imax(ss->start - 8, 0); maxLoc = imin(ss->stop + 8, maxIndex);
                    n = final_fill(M, which, 6, bases, L, ss, minLoc, maxLoc, 0, sc, mx, &job); haveMax = 1;
                }
            }
        }
        if (haveMax) {
            /* traceback of the last fill (the matrix holds nothing else); msa.rows / columns are whatever fillLimitedX left (the JNI
             * class's direct fillUnlimited does not set them, MultiStateAligner11tsJNI.java:178-192) */
            const int mlen = orc_traceback(msa, bases, ref, minLoc, maxLoc, mx[0], mx[1], mx[2], ss->ngaps ? 1 : 0, M->tb, M->tbcap);
            const int id = m_new(M, mlen > 0 ? mlen : 0);
            if (mlen > 0) memcpy(M->ms[id - 1].p, M->tb, (size_t)mlen);
            SITE_MATCH(ss) = id;
            set_limits(ss, sc[1], sc[2]);
            fix_limits_xy(M, ss);
            set_slow_score(ss, sc[0]);
            ss->match_job = job;                           /* (bookkeeping of this restatement: the fill the site's limits come from) */
        } else {
            set_stop(ss, ss->start + L - 1);
            set_slow_score(ss, scoreNoIndel);
        }
    }
    const int leftPad = left_padding_needed(M, ss, 4, 5), rightPad = right_padding_needed(M, ss, 4, 5);
    if (ss->stop < maxIndex && ss->start > 0 && (leftPad > 0 || rightPad > 0)) {
        if (recur > 0) {
            g_branch[4]++;
            fix_gaps(ss, ss->start, ss->stop);
            const int p_temp = imin(10 + imax(leftPad, rightPad), (msa->maxColumns - L) / 2 - 20);
            realign_new(M, which, ss, bases, L, p_temp, recur - 1, minValidScore, forbidIndels, fixXY);
        } else if (fixXY && match_contains_xy(M, ss)) fix_xy(M, ss, bases, L);
    }
    site_set_perfect(ss, bases, L, M->ix);
}

/* genMatchStringForSite (AbstractMapThread.java:968-1068), GEN_MATCH_FAST branch, secondary = false */
static void gen_match_string_for_site(mapper *M, int which, orc_msite *ss, const rstate *r, int maxSw, int paired) {
    const orc_map_params *P = M->P;
    const uint8_t *bases = ss->strand ? r->bm : r->bp; const int L = r->L;
    const float mult = paired ? orc_ratio_paired(P->minRatio) : P->minRatio;
    const int minMsaLimit = -1 + (int)(mult * (float)maxSw);
    if (ss->perfect) {
        const int id = m_new(M, L); memset(M->ms[id - 1].p, 'm', (size_t)L); SITE_MATCH(ss) = id;
    } else {
        const int oldScore = ss->slowScore;
        const int padding = (ss->perfect || ss->semiperfect) ? 0 : imax(P->slowAlignPadding, 6);
        realign_new(M, which, ss, bases, L, padding, 1, minMsaLimit, M->ix->p.maxIndel < 1, 0);
        fix_gaps(ss, ss->start, ss->stop);
        const int leftPad = left_padding_needed(M, ss, 4, 5), rightPad = right_padding_needed(M, ss, 4, 5);
        if (ss->slowScore < oldScore || leftPad > 0 || rightPad > 0) {
            int extra = (M->ix->p.maxIndel > 0 ? 80 : 20) + P->slowAlignPadding;
            const int expectedLen = calc_gref_len(ss);
            const int remaining = (M->msa->maxColumns - expectedLen - 2);
            extra = imax(0, imin(remaining / 2, extra));
            g_branch[5]++;
            realign_new(M, which, ss, bases, L, extra, 2, minMsaLimit, 0, 1);
            fix_gaps(ss, ss->start, ss->stop);
        }
        if (maxSw == ss->slowScore) ss->perfect = ss->semiperfect = 1;        /* SiteScore.setPerfectFlag (:227-233) */
        else site_set_perfect(ss, bases, L, M->ix);
    }
    clip_tip_indels(M, ss, bases, L, 4, 10);
}

/* ------------------------------------------------------------------ Read setters */
static void r_clear_site(rstate *r) { r->chrom = -1; r->strand = 0; r->start = -1; r->stop = -1; r->mapScore = 0; r->ngaps = 0; }
static void r_clear_mapping(rstate *r, slist *l, rstate *mate) {              /* Read.clearMapping (:1269-1276) */
    r_clear_site(r); r->match = 0; l->n = 0; r->mapped = 0; r->paired = 0;
    if (mate) mate->paired = 0;
}
static void r_set_from_site(rstate *r, orc_msite *ss) {                       /* Read.setFromSite (:1172-1190) */
    r->chrom = ss->chrom; r->strand = ss->strand; r->start = ss->start; r->stop = ss->stop; r->mapScore = ss->slowScore;
    r->rescued = ss->rescued; r->perfect = ss->perfect; r->match = SITE_MATCH(ss);
    if (ss->ngaps) fix_gaps(ss, r->start, r->stop);
    r->ngaps = ss->ngaps; memcpy(r->gaps, ss->gaps, sizeof r->gaps);
}
static void r_set_from_top_site(rstate *r, slist *l) {                        /* Read.setFromTopSite(false, true, .) (:1213-1225) */
    if (l->n == 0) { r_clear_site(r); r->mapped = 0; return; }
    r->mapped = 1;
    r_set_from_site(r, &l->s[0]);
}
static int contains_xyc(mapper *M, const rstate *r) {                          /* Read.containsXYC (:2051-2056) */
    const mstr *m = m_get(M, r->match);
    if (!m || m->len < 1) return 0;
    return m->p[0] == 'X' || m->p[m->len - 1] == 'Y' || m->p[0] == 'C' || m->p[m->len - 1] == 'C';
}

/* Tools.mergeDuplicateSites(list, false, false) (Tools.java:697-759): only exact positional matches (gaps included) merge */
static void merge_duplicate_sites_exact(slist *l) {
    if (l->n < 2) return;
    sort_list(l, cmp_pos);
    uint8_t dead[LISTCAP]; memset(dead, 0, (size_t)l->n);
    int removed = 0, ai = 0;
    for (int i = 1; i < l->n; i++) {
        orc_msite *a = &l->s[ai], *b = &l->s[i];
        if (positional_match(a, b, 1)) {
            set_slow_score(a, imax(a->slowScore, b->slowScore));
            a->pairedScore = (a->pairedScore <= a->slowScore && b->pairedScore <= a->slowScore) ? 0 : max3(0, a->pairedScore, b->pairedScore);
            a->score = imax(a->score, b->score);
            a->perfect = (a->perfect || b->perfect);
            a->semiperfect = (a->semiperfect || b->semiperfect);
            removed++; dead[i] = 1;
        } else ai = i;
    }
    if (removed) condense(l, dead);
}
static int check_order(const slist *l) {                                       /* Read.CHECKORDER (:3141-3150) */
    for (int i = 1; i < l->n; i++) if (l->s[i].score > l->s[i - 1].score) return 0;
    return 1;
}
static void remove_at(slist *l, int i) { for (int j = i + 1; j < l->n; j++) l->s[j - 1] = l->s[j]; l->n--; }

/* genMatchString (AbstractMapThread.java:860-965); PRINT_SECONDARY_ALIGNMENTS = false */
static void gen_match_string(mapper *M, int which, rstate *r, rstate *mate, slist *l, int maxSw, int setSSScore, int paired) {
    if (l->n == 0) { r->chrom = -1; return; }
    int best = INT_MIN, scoreChanged = 0;
    for (int i = 0; i < l->n; i++) {
        orc_msite *ss = &l->s[i];
        if (i > 0 && best >= ss->slowScore) break;
        const int oldSlowScore = ss->slowScore, oldScore = ss->score;
        if (SITE_MATCH(ss) == 0) {
            if (i > 0) g_branch[8]++;
            gen_match_string_for_site(M, which, ss, r, maxSw, paired);
            if (setSSScore) ss->score = ss->slowScore;
        }
        if (i > 0 && SITE_MATCH(ss) == 0 && !r->paired) { remove_at(l, i); /* (the index then moves on, as in the reference) */ }
        else {
            if (oldScore != ss->score || oldSlowScore != ss->slowScore) scoreChanged++;
            best = imax(ss->slowScore, best);
        }
    }
    int needsSorting = (scoreChanged > 0 && !check_order(l));
    while (needsSorting) {
        needsSorting = 0; g_branch[6]++;
        const int topObj = SITE_OBJ(&l->s[0]);
        merge_duplicate_sites_exact(l);
        sort_list(l, cmp_score);
        /* `for(i=0; i<size && i<MAX_SITESCORES_TO_PRINT; i++)` with its `if(i>0 || !PRINT_SECONDARY_ALIGNMENTS){break;}`: only the top site */
        if (l->n > 0 && SITE_MATCH(&l->s[0]) == 0) {
            orc_msite *ss = &l->s[0];
            gen_match_string_for_site(M, which, ss, r, maxSw, paired);
            if (setSSScore) ss->score = ss->slowScore;
            needsSorting = 1;
        }
        if (r->paired && SITE_OBJ(&l->s[0]) != topObj) { r->paired = 0; if (mate) mate->paired = 0; }
    }
    orc_msite *ss = &l->s[0];
    r->start = ss->start; r->stop = ss->stop; r->chrom = ss->chrom; r->strand = ss->strand;
    r->match = SITE_MATCH(ss); r->ngaps = ss->ngaps; memcpy(r->gaps, ss->gaps, sizeof r->gaps);
    r->mapScore = ss->slowScore; r->perfect = ss->perfect; r->rescued = ss->rescued;
}

/* removeDuplicateBestSites (:1328-1349) */
static void remove_duplicate_best_sites(slist *l) {
    if (l->n < 2) return;
    const orc_msite ss1 = l->s[0];
    for (int i = l->n - 1; i > 0; i--) {
        const orc_msite *ss2 = &l->s[i];
        if (ss1.chrom == ss2->chrom && ss1.strand == ss2->strand && ss1.start == ss2->start && ss1.stop == ss2->stop) { g_branch[9]++; remove_at(l, i); }
        else break;
    }
}

/* MSA.toLocalAlignment(r, ss, basesM, minToClip, matchPointsMult = 1) (MSA.java:216-484) */
static int to_local_alignment(mapper *M, rstate *r, rstate *mate, slist *l, int minToClip) {
    orc_msite *ss = &l->s[0];
    const uint8_t *bases = (r->strand == 0 ? r->bp : r->bm); const int L = r->L;
    mstr *mm = m_get(M, r->match);
    if (!mm || mm->len < 1) return 0;
    g_branch[2]++;
    if (mm->p[0] == 'X' || mm->p[mm->len - 1] == 'Y') {            /* Read.containsXY2 */
        fix_xy(M, ss, bases, L);
        r->start = ss->start; r->stop = ss->stop;
    }
    uint8_t *match = mm->p; const int n = mm->len;
    int maxScore = -1, startLocC = -1, stopLocC = -1, lastZeroC = 0, startLocM = -1, stopLocM = -1, lastZeroM = 0;
    int startLocR = -1, stopLocR = -1, lastZeroR = 0;
    uint8_t mode = match[0], prevMode = '0';
    int current = 0, prevStreak = 0, cpos = 0, rpos = r->start, score = 0;
    for (int mpos = 0; mpos <= n; mpos++) {
        const int atEnd = (mpos == n);
        if (!atEnd && mode == match[mpos]) { current++; continue; }
        if (atEnd && current <= 0) break;
        if (mode == 'm') {
            if (score <= 0) { score = 0; lastZeroC = cpos; lastZeroM = mpos - current; lastZeroR = rpos; }
            score += (int)(1.0f * (float)(F_MATCH + (current - 1) * F_MATCH2));         /* score+=(matchPointsMult*add): int += float */
            cpos += current; rpos += current;
            if (score > maxScore) {
                maxScore = score; startLocC = lastZeroC; startLocM = lastZeroM; startLocR = lastZeroR;
                stopLocC = cpos - 1; stopLocM = mpos - 1; stopLocR = rpos - 1;
            }
        } else if (mode == 'S') {
            score += calc_sub_score(current);
            if (prevMode == 'N' || prevMode == 'R') score += F_SUB2 - F_SUB;
            else if (prevMode == 'm' && prevStreak < 2) score += F_SUBR - F_SUB;
            cpos += current; rpos += current;
        } else if (mode == 'D') { score += orc_calc_del_score(current, 1); rpos += current; }
        else if (mode == 'I') { score += orc_calc_ins_score(current); cpos += current; }
        else if (mode == 'C') { cpos += current; rpos += current; }
        else if (mode == 'X' || mode == 'Y') { score += orc_calc_ins_score(current); cpos += current; rpos += current; }
        else if (mode == 'N' || mode == 'R') { cpos += current; rpos += current; }
        if (atEnd) break;
        prevMode = mode; prevStreak = current; mode = match[mpos]; current = 1;
    }
    if (startLocC < 0 || stopLocC < 0) { r_clear_mapping(r, l, mate); return 0; }
    int headTrimR = startLocC, headTrimM = startLocM, tailTrimR = L - stopLocC - 1, tailTrimM = n - stopLocM - 1;
    if (headTrimR <= minToClip && headTrimM <= minToClip) headTrimR = headTrimM = 0;
    if (tailTrimR <= minToClip && tailTrimM <= minToClip) tailTrimR = tailTrimM = 0;
    if (headTrimR == 0 && headTrimM == 0 && tailTrimR == 0 && tailTrimM == 0) return 0;
    const int headDelta = headTrimR - headTrimM, tailDelta = tailTrimR - tailTrimM;
    int id2 = r->match;
    g_branch[3]++;
    if (headDelta == 0 && tailDelta == 0) {
        for (int i = 0; i < headTrimM; i++) match[i] = 'C';
        for (int i = n - tailTrimM; i < n; i++) match[i] = 'C';
    } else {
        const int newlen = n - headTrimM - tailTrimM + headTrimR + tailTrimR;
        id2 = m_new(M, newlen);
        mm = m_get(M, r->match); match = mm->p;
        uint8_t *match2 = M->ms[id2 - 1].p;
        for (int i = 0; i < headTrimR; i++) match2[i] = 'C';
        for (int i = newlen - tailTrimR; i < newlen; i++) match2[i] = 'C';
        for (int i = headTrimM, i2 = headTrimR, lim = newlen - tailTrimR; i2 < lim; i++, i2++) match2[i2] = match[i];
    }
    if (headTrimR != 0) r->start = startLocR - headTrimR;
    if (tailTrimR != 0) r->stop = stopLocR + tailTrimR;
    r->match = id2;
    maxScore = imax(maxScore, ss->slowScore);
    r->mapScore = maxScore;
    SITE_MATCH(ss) = r->match;
    set_limits(ss, r->start, r->stop);
    /* isPerfect / isSemiPerfect (SiteScore.java:175-223) */
    int32_t ps[2];
    orc_set_perfect(bases, L, M->ix->chromArr[ss->chrom], M->ix->chromArrLen[ss->chrom], ss->start, ss->stop, ps);
    int isPerfect = 0, isSemi = 0;
    if (L == ss->stop - ss->start + 1) {
        const uint8_t *ref = M->ix->chromArr[ss->chrom]; const int reflen = M->ix->chromArrLen[ss->chrom];
        if (ss->start >= 0 && ss->stop < reflen) { isPerfect = 1; for (int i = 0; i < L; i++) { const uint8_t c = bases[i], rr = ref[ss->start + i]; if (c != rr || c == 'N') { isPerfect = 0; break; } } }
        {
            int readStart = 0, readStop = L, maxNoref = L / 2; const int refStop = ss->start + L;
            if (ss->start < 0) readStart = -ss->start;
            if (refStop > reflen) readStop -= (refStop - reflen);
            isSemi = 1;
            for (int i = readStart; i < readStop; i++) {
                const uint8_t c = bases[i], rr = ref[ss->start + i];
                if (c == 'N') { isSemi = 0; break; }
                if (c != rr) { maxNoref--; if (maxNoref < 0 || rr != 'N') { isSemi = 0; break; } }
            }
        }
    }
    (void)ps;
    if (!ss->perfect && isPerfect) {
        ss->perfect = ss->semiperfect = 1; r->perfect = 1;
        mstr *m2 = m_get(M, r->match); memset(m2->p, 'm', (size_t)m2->len);
        set_slow_score(ss, maxScore);
    } else if (!ss->semiperfect && isSemi) {
        ss->semiperfect = 1;
        const int id3 = m_new(M, L);
        orc_gen_match_no_indels(bases, L, M->ix->chromArr[ss->chrom], M->ix->chromArrLen[ss->chrom], ss->start, M->ms[id3 - 1].p);
        r->match = SITE_MATCH(ss) = id3;
        return to_local_alignment(M, r, mate, l, minToClip);
    }
    return 1;
}

/* Tools.countTopScores (Tools.java:913-930) */
static int count_top_scores(const slist *l, int thresh) {
    if (l->n == 0) return 0;
    int count = 1; const orc_msite *ss = &l->s[0]; const int limit = ss->score - thresh;
    for (int i = 1; i < l->n; i++) {
        const orc_msite *ss2 = &l->s[i];
        if (ss2->score < limit) break;
        if (ss->start != ss2->start && ss->stop != ss2->stop) count++;
    }
    return count;
}
/* Tools.removeLowQualitySitesUnpaired (Tools.java:986-1003): never removes positions 0 and 1 */
static void remove_low_quality_unpaired(slist *l, int thresh) {
    if (l->n == 0) return;
    if (l->s[0].score < thresh) { l->n = 0; return; }
    for (int i = l->n - 1; i > 1; i--) if (l->s[i].slowScore < thresh) remove_at(l, i);
}
/* Read.setPerfectFlag(maxScore) (Read.java:2494-2512); Read.match is null here, so testMatchPerfection(false) = false */
static void r_set_perfect_flag(rstate *r, const slist *l, int maxScore) {
    if (l->n == 0) { r->perfect = 0; return; }
    r->perfect = (l->s[0].slowScore == maxScore || l->s[0].perfect) ? 1 : 0;
}

enum { CZ_LIMIT1E = 40 };                                  /* BBMapThread.java:44 */
static const float CZ3_MULTS[7] = {0.f, 1.f, .75f, 0.5f, 0.25f, 0.125f, 0.0625f};      /* AbstractMapThread.java:2809 */

/* applyClearzone3 (:1820-1870), calcCZ3_fraction (:1893-1910) */
static int apply_clearzone3(rstate *r, slist *l, int CZ3, float INV_CZ3) {
    if (!r->mapped || r->ambiguous || l->n < 2) return 0;
    const int score1 = l->s[0].slowScore;
    float sub = 0;
    const int max = imin(7, l->n);
    for (int i = 1; i < max; i++) {
        const orc_msite *ss2 = &l->s[i];
        if (i > 2 && ss2->slowScore < l->s[i - 1].slowScore) break;
        const int dif = score1 - ss2->slowScore;
        float f;
        if (dif >= CZ3) f = 0;
        else { const int dif2 = CZ3 - dif; const float g = (float)dif2 * INV_CZ3, g2 = g * g; f = g + 2.f * g2 + 2.f * g2 * g; }
        if (f <= 0) break;
        sub += (f * CZ3_MULTS[i]);
    }
    if (sub <= 0) return 0;
    const float asymptote = 4.f + 0.03f * (float)r->L;
    sub = sub * 1.8f;
    const float sub2 = (float)CZ3 * ((asymptote * sub) / (sub + asymptote));
    int subi = (int)(sub2 + 0.5f);
    if (subi >= r->mapScore - 300) subi = r->mapScore - 300;
    if (subi <= 0) return 0;
    for (int i = 0; i < l->n; i++) { set_slow_score(&l->s[i], l->s[i].slowScore - subi); l->s[i].score -= subi; }
    r->mapScore -= subi;
    return 1;
}

/* calcTipScorePenalty(r, maxScore, tiplen) (:2499-2573) */
static int calc_tip_score_penalty(mapper *M, const rstate *r, int maxScore, int tiplen) {
    const mstr *m = m_get(M, r->match);
    if (!r->mapped || !m || r->L < 2 * tiplen) return 0;
    int points = 0;
    const uint8_t *match = m->p, *bases = r->bp; const int last = r->L - 1;
    uint8_t prev = 'm';
    for (int i = 0, cpos = 0; cpos <= tiplen; i++) {
        const uint8_t b = match[i];
        if (b == 'm') cpos++;
        else if (b == 'D') { if (prev != 'D') points += 2 * (tiplen + 2 - cpos); }
        else if (b == 'N' || b == 'C') { points += (tiplen + 2 - cpos); cpos++; }
        else { points += 2 * (tiplen + 2 - cpos); cpos++; }
        prev = b;
    }
    prev = 'm';
    for (int i = m->len - 1, cpos = 0; cpos <= tiplen; i--) {
        const uint8_t b = match[i];
        if (b == 'm') cpos++;
        else if (b == 'D') { if (prev != 'D') points += 2 * (tiplen + 2 - cpos); }
        else if (b == 'N' || b == 'C') { points += (tiplen + 2 - cpos); cpos++; }
        else { points += 2 * (tiplen + 2 - cpos); cpos++; }
        prev = b;
    }
    uint8_t b = bases[0];
    if (b != 'N' && b == bases[1]) for (int i = 2; i <= tiplen && bases[i] == b; i++) points++;
    b = bases[last];
    if (b != 'N' && b == bases[last - 1]) for (int i = last - 2; i >= (last - tiplen) && bases[i] == b; i--) points++;
    if (points < 1) return 0;
    const float asymptote = 80;
    const float f = ((asymptote * (float)points) / ((float)points + asymptote));
    const int penalty = (int)(f * .0022f * (float)maxScore);
    const int maxPenalty = r->mapScore - maxScore / 10;
    if (maxPenalty <= 0) return 0;
    return imin(penalty, maxPenalty);
}

/* pairSiteScoresFinal(r, r2, trim = true, setScore = true, ...) (:1919-2095) */
static void pair_site_scores_final(mapper *M, slist *l1, slist *l2, int len1, int len2) {
    const orc_map_params *P = M->P;
    for (int i = 0; i < l1->n; i++) l1->s[i].pairedScore = 0;
    for (int i = 0; i < l2->n; i++) l2->s[i].pairedScore = 0;
    if (l1->n < 1 || l2->n < 1) return;
    sort_list(l1, cmp_pos); sort_list(l2, cmp_pos);
    int maxPairedScore1 = -1, maxPairedScore2 = -1;
    const float q1 = (float)len1 / (4.f * (float)len2), q2 = (float)len2 / (4.f * (float)len1);
    const float h1 = 0.25f > q1 ? 0.25f : q1, h2 = 0.25f > q2 ? 0.25f : q2;
    const float mult1 = 0.5f < h1 ? 0.5f : h1, mult2 = 0.5f < h2 ? 0.5f : h2;
    const int ilimit = l1->n - 1, jlimit = l2->n - 1;
    const int outerDistLimit = (imax(len1, len2) * OUTER_DIST_MULT) / OUTER_DIST_DIV;
    const int expectedFragLength = P->averagePairDist + len1 + len2;
    const int MPD = P->maxPairDist;
    for (int i = 0, j = 0; i <= ilimit && j <= jlimit; i++) {
        orc_msite *ss1 = &l1->s[i], *ss2 = &l2->s[j];
        while (j < jlimit && (ss2->chrom < ss1->chrom || (ss2->chrom == ss1->chrom && ss1->start - ss2->stop > MPD))) { j++; ss2 = &l2->s[j]; }
        for (int k = j; k <= jlimit; k++) {
            ss2 = &l2->s[k];
            if (ss2->chrom > ss1->chrom) break;
            if (ss2->start - ss1->stop > MPD) break;
            int innerdist, outerdist;
            if (ss1->strand != ss2->strand) {
                if (ss1->strand == 0) { innerdist = ss2->start - ss1->stop; outerdist = ss2->stop - ss1->start; }
                else { innerdist = ss1->start - ss2->stop; outerdist = ss1->stop - ss2->start; }
            } else if (ss1->start <= ss2->start) { innerdist = ss2->start - ss1->stop; outerdist = ss2->stop - ss1->start; }
            else { innerdist = ss1->start - ss2->stop; outerdist = ss1->stop - ss2->start; }
            if (outerdist >= outerDistLimit && innerdist <= MPD) {
                const int strandOK = (ss1->strand != ss2->strand);                  /* SAME_STRAND_PAIRS = false, REQUIRE_CORRECT_STRANDS_PAIRS = true */
                if (strandOK) {
                    const int deviation = iabsdif(P->averagePairDist, innerdist);
                    const int den = imax(100, (10 * expectedFragLength + 100));
                    const int ps1 = ss1->score + 1 + imax(1, (int)((float)ss2->score * mult1) - ((deviation * ss2->score) / den));
                    const int ps2 = ss2->score + 1 + imax(1, (int)((float)ss1->score * mult2) - ((deviation * ss1->score) / den));
                    ss1->pairedScore = imax(ss1->pairedScore, ps1);
                    ss2->pairedScore = imax(ss2->pairedScore, ps2);
                    maxPairedScore1 = imax(ss1->score, maxPairedScore1);
                    maxPairedScore2 = imax(ss2->score, maxPairedScore2);
                }
            }
        }
    }
    for (int i = 0; i < l1->n; i++) if (l1->s[i].pairedScore > l1->s[i].score) l1->s[i].score = l1->s[i].pairedScore;
    for (int i = 0; i < l2->n; i++) if (l2->s[i].pairedScore > l2->s[i].score) l2->s[i].score = l2->s[i].pairedScore;
    const float f = 0.95f;                                                           /* min(SECONDARY_SITE_SCORE_RATIO, 0.95f) */
    trim_below_cutoff(l1, (int)((float)maxPairedScore1 * f), 0, 1, 1, P->maxTrimSitesToRetain);
    trim_below_cutoff(l2, (int)((float)maxPairedScore2 * f), 0, 1, 1, P->maxTrimSitesToRetain);
}
/* canPair (:2097-2164) */
static int can_pair(const orc_msite *ss1, const orc_msite *ss2, int len1, int len2, int MPD) {
    if (ss1->chrom != ss2->chrom) return 0;
    if (ss1->strand == ss2->strand) return 0;
    const int outerDistLimit = (imax(len1, len2) * OUTER_DIST_MULT) / OUTER_DIST_DIV;
    int innerdist, outerdist;
    if (ss1->strand == 0) { innerdist = ss2->start - ss1->stop; outerdist = ss2->stop - ss1->start; }
    else { innerdist = ss1->start - ss2->stop; outerdist = ss1->stop - ss2->start; }
    return outerdist >= outerDistLimit && innerdist <= MPD;
}

static void r_init(rstate *r, const uint8_t *bp, const uint8_t *bm, int L, int64_t id) {
    memset(r, 0, sizeof *r); r->chrom = -1; r->start = -1; r->stop = -1; r->bp = bp; r->bm = bm; r->L = L; r->numericID = id;
}
static void tag_objects(slist *l) { for (int i = 0; i < l->n; i++) { l->s[i].reserved[0] = 0; l->s[i].reserved[1] = i + 1; } }

/* the clearzone of the single-ended flow (BBMapThread.java:508-525) and the one of the paired flow (:1158-1160) */
static int clearzone_single(const orc_map_params *P, int perfect, int score, int maxSw) {
    (void)P;
    const int CZ1 = (int)(2.0f * F_MATCH2), CZ1b = (int)(2.6f * F_MATCH2), CZ1c = (int)(4.6f * F_MATCH2), CZP = (int)(1.6f * F_MATCH2);
    if (perfect) return CZP;
    const float cz1blimit = ((float)maxSw * 0.97f - 12.f * F_MATCH2), cz1climit = ((float)maxSw * 0.92f - 26.f * F_MATCH2);
    if ((float)score > cz1blimit) return (int)(((float)((maxSw - score) * CZ1b) + ((float)score - cz1blimit) * (float)CZ1) / ((float)maxSw - cz1blimit));
    if ((float)score > cz1climit) return (int)(((cz1blimit - (float)score) * (float)CZ1c + ((float)score - cz1climit) * (float)CZ1b) / (cz1blimit - cz1climit));
    return CZ1c;
}
static int clearzone_paired(int perfect, int score, int maxSw) {
    const int CZ1 = (int)(2.0f * F_MATCH2), CZ1b = (int)(2.6f * F_MATCH2), CZ1c = (int)(4.6f * F_MATCH2), CZP = (int)(1.6f * F_MATCH2);
    if (perfect) return CZP;
    if (score >= (int)((float)maxSw * 0.97f - 12.f * F_MATCH2)) return CZ1;
    if (score >= (int)((float)maxSw * 0.92f - 26.f * F_MATCH2)) return CZ1b;
    return CZ1c;
}

/* BBMapThread.processRead, from `if(r.numSites()>1)` after the merge + sort to the end (:492-732) */
static void final_single(mapper *M, rstate *r, slist *l) {
    const orc_map_params *P = M->P;
    const int L = r->L, maxSw = orc_max_quality(L);
    tag_objects(l);
    r_set_perfect_flag(r, l, maxSw);
    if (l->n > 1) {
        const int score = l->s[0].score;
        const int clearzone = clearzone_single(P, r->perfect, score, maxSw);
        int numBest = count_top_scores(l, clearzone);
        if (numBest > 1) r->ambiguous = 1;
        else {
            const int lim = (r->perfect ? (int)(4.f * CZ_LIMIT1E) : score + CLEARZONE1E >= maxSw ? 2 * CZ_LIMIT1E : CZ_LIMIT1E) + 1;
            if (l->n > lim && clearzone < CLEARZONE1E) {
                numBest = count_top_scores(l, CLEARZONE1E);
                if (numBest > lim) r->ambiguous = 1;
            }
        }
    }
    if (l->n > 0) {
        const int lim = (int)((float)maxSw * P->minRatio);
        if (l->s[0].score < lim) l->n = 0;
        else remove_low_quality_unpaired(l, imin(lim, imax(1, lim - P->clearzone3)));
    }
    if (l->n == 0) r->mapScore = 0;
    r_set_from_top_site(r, l);
    if (l->n > 0) {                                                            /* MAKE_MATCH_STRING (:579-623) */
        if (SITE_MATCH(&l->s[0]) != 0) r->match = SITE_MATCH(&l->s[0]);
        else {
            int firstIter = 1;
            do {
                if (!firstIter) { g_branch[7]++; sort_list(l, cmp_score); r_set_from_top_site(r, l); }
                gen_match_string(M, 0, r, NULL, l, maxSw, 1, 0);
                l->s[0].score = l->s[0].slowScore;
                firstIter = 0;
            } while (l->n > 1 && l->s[0].score < l->s[1].score);
        }
    }
    if (l->n > 1) remove_duplicate_best_sites(l);
    if (l->n > 0) SITE_MATCH(&l->s[0]) = r->match;
    if (l->n > 0 && r->mapScore <= 0) { r->mapScore = 0; r->mapped = 0; l->n = 0; }                      /* :633-641 */
    if (r->mapScore > 0 && l->n == 0) r_clear_mapping(r, l, NULL);                                       /* :647-657 */
    else if (r->mapScore <= 0 && l->n > 0) r_clear_mapping(r, l, NULL);
    if (l->n > 0 && !r->ambiguous) {                                                                     /* :668-682 (CLEARZONE3 > CLEARZONE1) */
        const float cz3v2 = ((float)P->clearzone3 * (1.25f < ((float)maxSw / (float)r->mapScore) ? 1.25f : ((float)maxSw / (float)r->mapScore)));
        if (P->clearzone3 > 0 && apply_clearzone3(r, l, (int)cz3v2, 1 / cz3v2)) {
            const int minScore = (int)((float)maxSw * P->minRatio);
            if (r->mapScore < minScore) r->ambiguous = 1;
        }
    }
    if (r->mapped && contains_xyc(M, r)) to_local_alignment(M, r, NULL, l, 1);                           /* :692-695 */
    if (l->n == 0 || (!r->ambiguous && (float)r->mapScore < (float)maxSw * P->minRatio)) r_clear_mapping(r, l, NULL);      /* :697-699 */
    if (P->clearzone3 > 0) {                                                                             /* PENALIZE_AMBIG (:706-709) */
        const int penalty = calc_tip_score_penalty(M, r, maxSw, 7);
        if (penalty > 0) {
            r->mapScore -= penalty;
            for (int i = 0; i < l->n; i++) { set_slow_score(&l->s[i], l->s[i].slowScore - penalty); l->s[i].score -= penalty; }
        }
    }
}

/* BBMapThread.processReadPair from :1116 to the end */
static void final_pair(mapper *M, rstate *r1, rstate *r2, slist *l1, slist *l2) {
    const orc_map_params *P = M->P;
    const int len1 = r1->L, len2 = r2->L, maxSw1 = orc_max_quality(len1), maxSw2 = orc_max_quality(len2);
    if (l1->n > 1) sort_list(l1, cmp_score);
    if (l2->n > 1) sort_list(l2, cmp_score);
    remove_low_quality_paired(l1, maxSw1, P->minRatio, orc_ratio_paired(P->minRatio));
    remove_low_quality_paired(l2, maxSw2, P->minRatio, orc_ratio_paired(P->minRatio));
    pair_site_scores_final(M, l1, l2, len1, len2);
    if (l1->n > 0) sort_list(l1, cmp_score);
    if (l2->n > 0) sort_list(l2, cmp_score);
    tag_objects(l1); tag_objects(l2);
    r_set_perfect_flag(r1, l1, maxSw1); r_set_perfect_flag(r2, l2, maxSw2);
    if (l1->n > 1 && count_top_scores(l1, clearzone_paired(r1->perfect, l1->s[0].score, maxSw1)) > 1) r1->ambiguous = 1;
    if (l2->n > 1 && count_top_scores(l2, clearzone_paired(r2->perfect, l2->s[0].score, maxSw2)) > 1) r2->ambiguous = 1;
    if (l1->n > 0 && l2->n > 0 && can_pair(&l1->s[0], &l2->s[0], len1, len2, P->maxPairDist)) { r1->paired = 1; r2->paired = 1; }
    if (l1->n == 0) r1->mapScore = 0;
    if (l2->n == 0) r2->mapScore = 0;
    r_set_from_top_site(r1, l1); r_set_from_top_site(r2, l2);
    if (l1->n > 0) { if (SITE_MATCH(&l1->s[0]) != 0) r1->match = SITE_MATCH(&l1->s[0]); else gen_match_string(M, 0, r1, r2, l1, maxSw1, 0, 1); }
    if (l2->n > 0) { if (SITE_MATCH(&l2->s[0]) != 0) r2->match = SITE_MATCH(&l2->s[0]); else gen_match_string(M, 1, r2, r1, l2, maxSw2, 0, 1); }
    if (r1->mapScore > 0 && l1->n == 0) { r_clear_mapping(r1, l1, r2); }                                /* :1262-1272 */
    else if (r1->mapScore <= 0 && l1->n > 0) { r_clear_mapping(r1, l1, r2); }
    if (r2->mapScore > 0 && l2->n == 0) { r_clear_mapping(r2, l2, r1); }                                /* :1275-1285 */
    else if (r2->mapScore <= 0 && l2->n > 0) { r_clear_mapping(r2, l2, r1); }
    remove_duplicate_best_sites(l1); remove_duplicate_best_sites(l2);
    if (r1->mapped && contains_xyc(M, r1)) { SITE_MATCH(&l1->s[0]) = r1->match; to_local_alignment(M, r1, r2, l1, 1); }    /* :1334-1340 */
    if (r2->mapped && contains_xyc(M, r2)) { SITE_MATCH(&l2->s[0]) = r2->match; to_local_alignment(M, r2, r1, l2, 1); }    /* :1344-1349 */
}

static void store_final(mapper *M, const rstate *r, const slist *l, orc_final *out, uint8_t *fmatch, int fstride) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->mapped = r->mapped; out->chrom = r->chrom; out->strand = r->strand; out->start = r->start; out->stop = r->stop;
    out->mapScore = r->mapScore; out->paired = r->paired; out->ambiguous = r->ambiguous; out->perfect = r->perfect; out->rescued = r->rescued;
    out->nsites = l->n;
    const mstr *m = m_get(M, r->match);
    out->match_len = m ? m->len : 0;
    if (m && fmatch && m->len <= fstride) memcpy(fmatch, m->p, (size_t)m->len);
}
